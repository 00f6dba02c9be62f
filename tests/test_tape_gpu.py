"""The training tape (goal_force_amd/training.py) per row on the device: gf_transpose_pad(_batched) through the raw C ABI, linear_dx /
linear_dw / bias_grad and the small autograd functions against fp64, DiTBlockFn.backward and the whole training step against fp64 autograd
of the oracle through the row statistic of tests/tape_refs.py.  Every threshold comes from that helper, where it is measured on two CPU
restatements against fp64 (tests/test_tape_refs_cpu.py) — none was read off the device.  `pytest -s` prints every ratio (lines `ROW`)."""
import functools
import math

import pytest
import torch

import attention_bwd_refs as AB
import backward_refs as BR
import forward_refs as FR
import gemm_refs as GR
import tape_refs as T

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN_BITS = 0x7FC1                 # a quiet-NaN bf16 pattern no kernel writes (as int16)
GUARD = 96                        # sentinel elements in front of and behind the destination


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from goal_force_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _grad_enabled():
    """Other test modules switch autograd off process-wide at import; the tape needs it."""
    with torch.enable_grad():
        yield


def _lib(ops):
    return ops._lib.load()


def _err(ops):
    return _lib(ops).gf_last_error().decode("utf-8", "replace")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16)


def _c(t):
    return None if t is None else t.cuda()


# ---------------------------------------------------------------------------------------------------------------------
# a. the transposes, raw C ABI
TR_R = (1, 7, 31, 32, 33, 63, 64, 65, 129)
TR_C = (1, 8, 12, 63, 64, 72, 136)


def _rpads(R):
    return sorted({R, -(-R // 8) * 8, -(-R // 64) * 64, R + 1})


def _transpose_case(ops, R, C, rpad, batch=1, layout="single", ld_extra=8, src_off=0, dst_off=0, stride_dst_extra=0, stride_src_extra=0):
    """One call of gf_transpose_pad (batch == 1 and layout 'single') or gf_transpose_pad_batched, checked bit for bit.
    layout: 'single' | 'side' (matrices side by side in one [R, batch C] tensor) | 'apart' (whole matrices apart) | 'same' (stride 0)."""
    g = torch.Generator().manual_seed(1009 * R + 31 * C + rpad + 7 * batch)
    nmat = 1 if layout in ("single", "same") else batch
    vals = torch.randint(-32768, 32768, (nmat, R, C), generator=g, dtype=torch.int32).to(torch.int16)      # any bit pattern, NaNs included
    if layout == "side":
        ld = batch * C + ld_extra
        parent = torch.full((R * ld + src_off + 8,), NAN_BITS, dtype=torch.int16)
        view = parent[src_off:src_off + R * ld].view(R, ld)
        for b in range(batch):
            view[:, b * C:(b + 1) * C] = vals[b]
        stride_src = C
    else:
        ld = C + ld_extra
        per = R * ld + stride_src_extra
        parent = torch.full((nmat * per + src_off + 8,), NAN_BITS, dtype=torch.int16)
        for b in range(nmat):
            parent[src_off + b * per:src_off + b * per + R * ld].view(R, ld)[:, :C] = vals[b]
        stride_src = 0 if layout in ("single", "same") else per
    stride_dst = C * rpad + stride_dst_extra
    dst = torch.full((GUARD + dst_off + batch * stride_dst + GUARD,), NAN_BITS, dtype=torch.int16)
    psrc, pdst = parent.cuda(), dst.cuda()
    sp = psrc.data_ptr() + 2 * src_off
    dp = pdst.data_ptr() + 2 * (GUARD + dst_off)
    lib = _lib(ops)
    if layout == "single":
        rc = lib.gf_transpose_pad(sp, ld, dp, R, C, rpad, _st())
    else:
        rc = lib.gf_transpose_pad_batched(sp, ld, stride_src, dp, stride_dst, R, C, rpad, batch, _st())
    what = f"transpose R={R} C={C} rpad={rpad} batch={batch} {layout} ld={ld} src_off={src_off} dst_off={dst_off} stride_dst={stride_dst}"
    assert rc == 0, f"{what}: {_err(ops)}"
    out = pdst.cpu()
    lo = GUARD + dst_off
    assert bool((out[:lo] == NAN_BITS).all()) and bool((out[lo + batch * stride_dst:] == NAN_BITS).all()), f"{what}: a sentinel around dst was written"
    for b in range(batch):
        m = out[lo + b * stride_dst:lo + (b + 1) * stride_dst]
        body, gap = m[:C * rpad].view(C, rpad), m[C * rpad:]
        want = vals[b if nmat > 1 else 0].t()
        assert torch.equal(body[:, :R], want), f"{what}: matrix {b} is not src.t()"
        assert bool((body[:, R:] == 0).all()), f"{what}: matrix {b}: columns [R, rpad) are not exactly +0"
        assert bool((gap == NAN_BITS).all()), f"{what}: the gap behind matrix {b} was written"


@pytest.mark.parametrize("R", TR_R)
def test_transpose_pad_every_shape_bit_for_bit(ops, R):
    """src a column slice of a NaN parent (ld = C + 8), dst poisoned and guarded: C % 8 == 0 with rpad % 8 == 0 runs the 64 x 64 kernel,
    everything else the 32 x 32 one."""
    for C in TR_C:
        for rpad in _rpads(R):
            _transpose_case(ops, R, C, rpad)


@pytest.mark.parametrize("why,kw", [("ld_src % 8", dict(ld_extra=4)), ("src at a 2-byte offset", dict(src_off=1)),
                                    ("dst at a 2-byte offset", dict(dst_off=1)), ("aligned", dict())])
def test_transpose_pad_each_reason_for_the_two_byte_kernel(ops, why, kw):
    for R, C, rpad in ((65, 72, 128), (129, 136, 136), (64, 64, 64)):
        _transpose_case(ops, R, C, rpad, **kw)
        _transpose_case(ops, R, C, rpad, batch=3, layout="apart", **kw)


@pytest.mark.parametrize("batch", [1, 3, 40])
def test_transpose_pad_batched_layouts(ops, batch):
    for R, C, rpad in ((65, 72, 128), (33, 12, 40), (129, 64, 130), (7, 8, 8), (64, 136, 64)):
        for layout in ("side", "apart", "same"):
            _transpose_case(ops, R, C, rpad, batch=batch, layout=layout)
            _transpose_case(ops, R, C, rpad, batch=batch, layout=layout, stride_dst_extra=40)          # a guarded gap behind every matrix
    _transpose_case(ops, 65, 72, 128, batch=batch, layout="apart", stride_src_extra=4)                  # stride_src % 8
    _transpose_case(ops, 65, 72, 128, batch=batch, layout="apart", stride_dst_extra=4)                  # stride_dst % 8
    _transpose_case(ops, 65, 12, 128, batch=batch, layout="side", ld_extra=4)                           # heads of 12 columns: nothing aligned


def test_transpose_pad_refusals_leave_the_destination_untouched(ops):
    lib = _lib(ops)
    src = torch.zeros((8, 16), dtype=BF, device="cuda")
    dst = torch.full((16 * 8 * 3,), NAN_BITS, dtype=torch.int16, device="cuda")
    s, d, st = src.data_ptr(), dst.data_ptr(), _st()
    single = [(None, 16, d, 8, 16, 8), (s, 16, None, 8, 16, 8), (s, 16, d, 0, 16, 8), (s, 16, d, 8, 0, 8), (s, 16, d, 8, 16, 7), (s, 15, d, 8, 16, 8)]
    for a in single:
        assert lib.gf_transpose_pad(*a, st) != 0, a
        assert "gf_transpose_pad: bad arguments" in _err(ops), (a, _err(ops))
    batched = [(None, 16, 128, d, 128, 8, 16, 8, 1), (s, 16, 128, None, 128, 8, 16, 8, 1), (s, 16, 128, d, 128, 0, 16, 8, 1),
               (s, 16, 128, d, 128, 8, 0, 8, 1), (s, 16, 128, d, 128, 8, 16, 7, 1), (s, 15, 128, d, 128, 8, 16, 8, 1),
               (s, 16, 128, d, 128, 8, 16, 8, 0), (s, 16, 0, d, 128, 8, 16, 8, 65536), (s, 16, -1, d, 128, 8, 16, 8, 1),
               (s, 16, 0, d, 127, 8, 16, 8, 2)]
    for a in batched:
        assert lib.gf_transpose_pad_batched(*a, st) != 0, a
        assert "gf_transpose_pad_batched: bad arguments" in _err(ops), (a, _err(ops))
    torch.cuda.synchronize()
    assert bool((dst == NAN_BITS).all()), "a refused call wrote to the destination"


# ---------------------------------------------------------------------------------------------------------------------
# b. linear_dx, linear_dw, bias_grad, LinearFn
def _poison(*shapes):
    """Allocate, fill with NaN and free buffers of these shapes: the next torch.empty of such a size gets poisoned memory."""
    bufs = [torch.full(s, math.nan, dtype=BF, device="cuda") for s in shapes]
    torch.cuda.synchronize()
    del bufs


def _check_linear(cls, M, got_dx, got_dw, x, w, dy, what):
    rdx, rdw, _ = T.linear_refs(x, w, dy)
    if cls == "gauss":
        GR.assert_pinned(got_dx.cpu(), rdx, w.shape[0], f"{what} dX")
        GR.assert_pinned(got_dw.cpu(), rdw, T.pad64(M), f"{what} dW")
        return
    assert torch.equal(got_dx.cpu().double(), rdx.out), f"{what} dX ({cls}) differs from the exact product"
    dwc = got_dw.cpu().double()
    if cls == "selector":
        col = T.selector_col(M, w.shape[0])
        want_rows = dy[torch.arange(M), col].double()[:, None] * x.double()
        for m in range(M):
            assert torch.equal(dwc[col[m]], want_rows[m]), f"{what} dW row {int(col[m])} is not dy[{m}, {int(col[m])}] x[{m}]"
    assert torch.equal(dwc, rdw.out), f"{what} dW ({cls}) differs from the exact product"


@pytest.mark.parametrize("M", T.LIN_M)
def test_linear_dx_dw_against_the_fp64_product(ops, M):
    from goal_force_amd import training as tr
    for cls in T.LIN_CLASSES:
        x, w, dy = T.linear_inputs(cls, M)
        xg = AB.embed(x.cuda(), 3, 24)                                           # a strided view in a NaN parent, as a saved activation
        wg, dyg = w.cuda(), dy.cuda()
        dx = tr.linear_dx(dyg, wg)
        mp = T.pad64(M)
        _poison((T.LIN_N, mp), (T.LIN_K, mp))
        dw = tr.linear_dw(dyg, xg)
        assert dx.dtype == BF and dw.dtype == BF and dx.shape == x.shape and dw.shape == w.shape
        _check_linear(cls, M, dx, dw, x, w, dy, f"linear {cls} M={M}")


@pytest.mark.parametrize("rows", T.BIAS_ROWS)
def test_bias_grad_against_the_fp64_column_sum(ops, rows):
    from goal_force_amd import training as tr
    for cols in T.BIAS_COLS:
        g = torch.Generator().manual_seed(100 * rows + cols)
        for cls, dy in (("gauss", torch.randn((rows, cols), generator=g).to(BF)),
                        ("integers", torch.randint(-1, 2, (rows, cols), generator=g).float().clamp(-1, 1).to(BF))):
            if cls == "integers" and rows > 256:
                dy[256:] = 0                                                     # |sum| <= 256: exactly representable
            got = tr.bias_grad(dy.cuda()).cpu().double()
            want, lo, hi = T.bias_grad_bound(dy)
            if cls == "integers":
                assert torch.equal(got, dy.double().sum(0)), (rows, cols)
            bad = ~((got >= lo) & (got <= hi))
            assert not bool(bad.any()), f"bias_grad ({rows}, {cols}) {cls}: columns {torch.nonzero(bad).flatten()[:4].tolist()} outside bf16(sum +- 1e-5 sum|dy|)"


def test_linear_dx_refuses_out_features_that_are_no_multiple_of_64(ops):
    from goal_force_amd import training as tr
    from goal_force_amd._lib import GoalForceError
    with pytest.raises(GoalForceError, match="multiple of 64"):
        tr.linear_dx(torch.zeros((4, 72), dtype=BF, device="cuda"), torch.zeros((72, 64), dtype=BF, device="cuda"))


def test_linear_fn_needs_input_grad_combinations(ops):
    from goal_force_amd.training import LinearFn
    x, w, dy = T.linear_inputs("gauss", 65, 128, 192, seed=1)                   # the forward GEMM's K is a multiple of 64
    b = (0.1 * torch.randn(128, generator=torch.Generator().manual_seed(2))).to(BF)
    full = None
    for mask in (7, 1, 2, 4, 3, 5, 6):
        leaves = [t.cuda().requires_grad_(bool(mask >> i & 1)) for i, t in enumerate((x, w, b))]
        LinearFn.apply(*leaves).backward(dy.cuda())
        grads = [t.grad for t in leaves]
        if full is None:
            full = grads
            rdx, rdw, _ = T.linear_refs(x, w, dy)
            GR.assert_pinned(full[0].cpu(), rdx, 128, "LinearFn dX")
            GR.assert_pinned(full[1].cpu(), rdw, T.pad64(65), "LinearFn dW")
            _, lo, hi = T.bias_grad_bound(dy)
            assert bool(((full[2].cpu().double() >= lo) & (full[2].cpu().double() <= hi)).all())
        for i, gr in enumerate(grads):
            if mask >> i & 1:
                assert gr is not None and torch.equal(_bits(gr), _bits(full[i])), (mask, i)
            else:
                assert gr is None, (mask, i)
    xg, wg = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)          # no bias: two gradients, the third slot None
    LinearFn.apply(xg, wg, None).backward(dy.cuda())
    assert torch.equal(_bits(xg.grad), _bits(full[0])) and torch.equal(_bits(wg.grad), _bits(full[1]))


# ---------------------------------------------------------------------------------------------------------------------
# c. the small functions
def _patch_inputs(cls, grid, seed):
    f, h, w = grid
    S = f * h * w
    g = torch.Generator().manual_seed(seed)
    shape = (T.PATCH_IN, f, 2 * h, 2 * w)
    if cls == "integers":
        lat, dy = torch.randint(-2, 3, shape, generator=g).float(), torch.randint(-1, 2, (S, T.PATCH_OUT), generator=g).float()
    elif cls == "selector":
        lat = GR._band_bf16(shape, g).float()
        dy = torch.zeros((S, T.PATCH_OUT))
        sign = torch.randint(0, 2, (S,), generator=g).float() * 2 - 1
        dy[torch.arange(S), T.selector_col(S, T.PATCH_OUT)] = sign * torch.exp2(torch.randint(-2, 3, (S,), generator=g).float())
    else:
        lat, dy = torch.randn(shape, generator=g), torch.randn((S, T.PATCH_OUT), generator=g)
    wt = (torch.randn((T.PATCH_OUT, T.PATCH_IN, 1, 2, 2), generator=g) / 12).to(BF)
    bias = (0.1 * torch.randn(T.PATCH_OUT, generator=g)).to(BF)
    return lat.to(BF), wt, bias, dy.to(BF)


def _conv_grads(lat, wt, dy, grid):
    """(dW, db) of F.conv3d (kernel = stride = (1, 2, 2)) on the un-gathered latent by fp64 autograd; dy [S, out] token-major."""
    f, h, w = grid
    wd = wt.double().requires_grad_(True)
    bd = torch.zeros(wt.shape[0], dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv3d(lat.double()[None], wd, bd, stride=(1, 2, 2))
    y.backward(dy.double().t().reshape(1, -1, f, h, w))
    return wd.grad, bd.grad


@pytest.mark.parametrize("grid", T.PATCH_GRIDS)
def test_patch_embed_fn_against_conv3d_autograd(ops, grid):
    from goal_force_amd.training import PatchEmbedFn
    S = grid[0] * grid[1] * grid[2]
    kpad = T.pad64(4 * T.PATCH_IN)
    assert kpad == 192
    for cls in T.LIN_CLASSES:
        lat, wt, bias, dy = _patch_inputs(cls, grid, 11 + S)
        cols = ops.patchify_im2col(lat.cuda().contiguous(), None, kpad=kpad)
        wg, bg = wt.cuda().requires_grad_(True), bias.cuda().requires_grad_(True)
        _poison((T.PATCH_OUT, T.pad64(S)), (kpad, T.pad64(S)))
        PatchEmbedFn.apply(cols, wg, bg).backward(dy.cuda())
        dw64, db64 = _conv_grads(lat, wt, dy, grid)
        assert wg.grad.shape == wt.shape and wg.grad.dtype == BF
        what = f"PatchEmbedFn {cls} grid {grid}"
        if cls == "gauss":
            s64 = _conv_grads(lat.abs(), wt, dy.abs(), grid)[0]
            ref = GR.Ref(*GR.chain(dw64.reshape(T.PATCH_OUT, -1), None, GR.EPI_BIAS, None, None, None, s64.reshape(T.PATCH_OUT, -1)), None, None)
            GR.assert_pinned(wg.grad.cpu().reshape(T.PATCH_OUT, -1), ref, T.pad64(S), what + " dW")
        else:
            assert torch.equal(wg.grad.cpu().double(), dw64), what + " dW differs from the exact gradient"
        _, lo, hi = T.bias_grad_bound(dy)
        got = bg.grad.cpu().double()
        assert bool(((got >= lo) & (got <= hi)).all()), what + " db"
        if cls != "gauss":
            assert torch.equal(got, FR.rb(db64)), what + " db"


@pytest.mark.parametrize("M", [1, 65, 130])
def test_inject_fn(ops, M):
    from goal_force_amd.training import InjectFn
    D = 192                                                                      # a multiple of 64, and >= every M (the selector class)
    for cls in T.LIN_CLASSES:
        state, w, dout = T.linear_inputs(cls, M, D, D, seed=3)
        g = torch.Generator().manual_seed(M)
        x2, b = torch.randn((M, D), generator=g).to(BF), (0.1 * torch.randn(D, generator=g)).to(BF)
        leaves = [t.cuda().requires_grad_(True) for t in (x2, state, w, b)]
        _poison((D, T.pad64(M)), (D, T.pad64(M)))
        dg = dout.cuda()
        InjectFn.apply(*leaves).backward(dg)
        assert torch.equal(_bits(leaves[0].grad), _bits(dg)), "InjectFn: the residual's gradient is dout itself"
        _check_linear(cls, M, leaves[1].grad, leaves[2].grad, state, w, dout, f"InjectFn {cls} M={M}")
        _, lo, hi = T.bias_grad_bound(dout)
        got = leaves[3].grad.cpu().double()
        assert bool(((got >= lo) & (got <= hi)).all())
        # a zero conv at its initial value: dstate exactly zero, dW and db as before
        zl = [leaves[0].detach().requires_grad_(True), leaves[1].detach().requires_grad_(True),
              torch.zeros_like(leaves[2]).requires_grad_(True), torch.zeros_like(leaves[3]).requires_grad_(True)]
        InjectFn.apply(*zl).backward(dg)
        assert not bool(zl[1].grad.any()), "zero weight: dstate must be exactly zero"
        assert torch.equal(_bits(zl[2].grad), _bits(leaves[2].grad)) and torch.equal(_bits(zl[3].grad), _bits(leaves[3].grad))


def test_fanout_fn(ops):
    from goal_force_amd.training import FanoutFn
    g = torch.Generator().manual_seed(8)
    x = torch.randn((65, 264), generator=g).to(BF).cuda().requires_grad_(True)
    g1, g2 = (torch.randn((65, 264), generator=g).to(BF) for _ in range(2))
    a, b = FanoutFn.apply(x)
    assert torch.equal(a, x) and torch.equal(b, x)
    torch.autograd.backward([a, b], [g1.cuda(), g2.cuda()])
    assert torch.equal(_bits(x.grad.cpu()), _bits((g1.float() + g2.float()).to(BF))), "FanoutFn: bf16(g1 + g2), one rounding"
    assert FanoutFn.backward(None, None, g2) is g2 and FanoutFn.backward(None, g1, None) is g1


@pytest.mark.parametrize("grid", T.PATCH_GRIDS)
def test_unpatchify_fn_backward_is_the_inverse_permutation(ops, grid):
    from goal_force_amd.training import UnpatchifyFn
    from oracle import wan_oracle as wo
    f, h, w = grid
    c = 16
    g = torch.Generator().manual_seed(f + h + w)
    tok = torch.randint(-100, 101, (f * h * w, 4 * c), generator=g).float().to(BF)
    dout = torch.randint(-100, 101, (c, f, 2 * h, 2 * w), generator=g).float().to(BF)
    tg = tok.cuda().requires_grad_(True)
    out = UnpatchifyFn.apply(tg, c, f, h, w)
    assert torch.equal(out.cpu().double(), wo.unpatchify(tok.double()[None], grid, c)[0])
    out.backward(dout.cuda())
    assert torch.equal(tg.grad.cpu().double(), T.unpatchify_bwd_ref(dout, c, f, h, w))


def test_mse_loss_fn(ops):
    from goal_force_amd.training import MseLossFn
    g = torch.Generator().manual_seed(9)
    pred, target = torch.randn((16, 3, 8, 12), generator=g).to(BF), torch.randn((16, 3, 8, 12), generator=g).to(BF)
    weight = 0.37
    _, dpred = ops.mse_loss(pred.cuda(), target.cuda(), weight=weight)
    BR.assert_within(dpred.cpu(), BR.mse_ref(pred, target, weight)[1], BR.mse_ref(pred, target, weight)[1].abs(), "mse dpred")
    grads = {}
    for up in (1.0, 0.5, 3.0):
        p = pred.cuda().requires_grad_(True)
        loss = MseLossFn.apply(p, target.cuda(), weight)
        (loss if up == 1.0 else loss * up).backward()
        grads[up] = p.grad.cpu()
    assert torch.equal(_bits(grads[1.0]), _bits(dpred.cpu())), "upstream 1.0: the kernel's dpred, bit for bit"
    assert torch.equal(grads[0.5].float(), dpred.cpu().float() * 0.5), "upstream 0.5: exact"
    want = FR.rb(3.0 * BR.mse_ref(pred, target, weight)[1]).to(BF)
    steps = int(FR.bf16_steps(grads[3.0], want).max())
    assert steps <= 1, f"upstream 3.0: {steps} bf16 steps from bf16(fp64)"


def test_layernorm_mod_fn_backward_is_the_kernel(ops):
    from goal_force_amd.training import LayerNormModFn
    x, dy, s1p = BR.row_inputs(65, 256, torch.Generator().manual_seed(10), "scale1p")
    shift = (0.1 * torch.randn(256, generator=torch.Generator().manual_seed(11))).to(BF)
    xg = x.cuda().requires_grad_(True)
    LayerNormModFn.apply(xg, s1p.cuda(), shift.cuda(), 1e-6).backward(dy.cuda())
    assert torch.equal(_bits(xg.grad), _bits(ops.layernorm_bwd(x.cuda(), dy.cuda(), g=s1p.cuda(), eps=1e-6)))


# ---------------------------------------------------------------------------------------------------------------------
# d. the block tape
CASES = {c["name"]: c for c in T.cases()}


@functools.lru_cache(maxsize=None)
def _case(name, zero_row=None):
    """(inputs, fp64 reference, restatement of order 0) of a case — computed once on the host and left unchanged."""
    import gen_inputs as gi
    case = CASES[name]
    cfg, sd, x, ctx, t_mod, dout = T.case_inputs(case, gi)
    if zero_row is not None:
        t_mod = T.zero_gate(sd, t_mod, zero_row)
    ref = T.with_dx(*T.block_grads_ref(cfg, sd, x, ctx, t_mod, dout, case["grid"]))
    c0 = T.with_dx(*T.block_chain(cfg, sd, x, ctx, t_mod, dout, case["grid"], 0, case["prescale"]))
    return (cfg, sd, x, ctx, t_mod, dout), ref, c0


def _run_block(ops, name, inputs, subset=T.PARAM_NAMES, level=None, monkeypatch=None):
    from goal_force_amd import training
    from goal_force_amd.dit import DiTBlock, RopeTable, precompute_freqs_cis_3d
    case = CASES[name]
    cfg, sd, x, ctx, t_mod, dout = inputs
    blk = DiTBlock(False, cfg["dim"], cfg["num_heads"], cfg["ffn_dim"], cfg["eps"])
    blk.load_state_dict(sd, strict=True)
    blk = blk.to(BF).cuda()
    for n, p_ in blk.named_parameters():
        p_.requires_grad_(n in subset)
    rope = RopeTable.from_grid(precompute_freqs_cis_3d(cfg["dim"] // cfg["num_heads"]), *case["grid"], "cuda")
    if level is not None:
        monkeypatch.setattr(training, "KEEP_ATTENTION", True)                  # (restores the module state after the test)
        monkeypatch.setattr(training, "KEEP_WIDE", False)
        monkeypatch.setattr(training, "KEEP_AUTO", True)
        training.set_keep_level(level)
    xc = x.cuda().requires_grad_(True)
    with ops.options(attn_q_prescale=case["prescale"]):
        y = training.block_forward(blk, xc, ctx.cuda(), t_mod.cuda(), rope)
        y.backward(dout.cuda())
    named = dict(blk.named_parameters())
    for n in T.PARAM_NAMES:
        assert (named[n].grad is not None) == (n in subset), f"{n}: .grad is {'missing' if n in subset else 'set although not asked for'}"
    got = {n: named[n].grad.cpu() for n in subset}
    got["dx"] = xc.grad.cpu()
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_block_tape_every_slice(ops, name):
    inputs, ref, c0 = _case(name)
    got = _run_block(ops, name, inputs)
    T.assert_rows(got, c0, ref, f"block tape {name}")


@pytest.mark.parametrize("level", ["none", "attn", "wide"])
def test_block_tape_at_every_keep_level(ops, level, monkeypatch):
    inputs, ref, c0 = _case(T.BASE_CASE)
    got = _run_block(ops, T.BASE_CASE, inputs, level=level, monkeypatch=monkeypatch)
    T.assert_rows(got, c0, ref, f"block tape keep={level}")


@pytest.mark.parametrize("subset", list(T.SUBSETS))
def test_block_tape_for_a_subset_of_the_parameters(ops, subset):
    inputs, ref, c0 = _case(T.BASE_CASE)
    got = _run_block(ops, T.BASE_CASE, inputs, subset=T.SUBSETS[subset])
    assert set(got) == set(T.SUBSETS[subset]) | {"dx"}
    T.assert_rows(got, c0, ref, f"block tape subset {subset}")


@pytest.mark.parametrize("row,branch,zero_rows", [(5, "ffn.", (3, 4)), (2, "self_attn.", (0, 1))])
def test_block_tape_exact_zeros_behind_a_zero_gate(ops, row, branch, zero_rows):
    inputs, ref, c0 = _case(T.BASE_CASE, row)
    got = _run_block(ops, T.BASE_CASE, inputs)
    for n in T.PARAM_NAMES:
        if n.startswith(branch):
            assert not bool(got[n].any()), f"{n} behind a zero gate is not exactly zero"
    m = got["modulation"].reshape(6, -1)
    assert not bool(m[list(zero_rows)].any()) and bool(m[row].any())
    T.assert_rows(got, c0, ref, f"block tape zero gate row {row}")


# ---------------------------------------------------------------------------------------------------------------------
# e. the whole tape, two ControlNet layers
@functools.lru_cache(maxsize=None)
def _model_case(zero):
    import gen_inputs as gi
    cfg, inp = gi.TINY, gi.train_inputs()
    dit_sd, cn_sd = gi.dit_sd(cfg, seed=41), gi.controlnet_sd(cfg, 2, seed=42, zero_convs_zero=zero)
    args = (cfg, dit_sd, cn_sd, 2, inp, gi.TRAIN_TIMESTEP_ID)
    return args, T.model_grads_ref(*args), T.model_chain(*args, order=0)


@pytest.mark.parametrize("zero", T.MODEL_CASES)
def test_whole_tape_with_two_controlnet_layers(ops, zero):
    import gen_inputs as gi
    from goal_force_amd.controlnet import ControlNet
    from goal_force_amd.dit import WanModel
    from goal_force_amd.pipeline import WanVideoPipeline
    (cfg, dit_sd, cn_sd, n_cn, inp, tid), (loss_ref, g_ref), (l0, c0) = _model_case(zero)
    dit = WanModel(has_image_input=False, require_clip_embedding=False, **cfg)
    dit.load_state_dict(dit_sd, strict=True)
    cn = ControlNet(n_cn, dim=cfg["dim"], num_heads=cfg["num_heads"], ffn_dim=cfg["ffn_dim"])
    cn.load_state_dict(cn_sd, strict=True)
    dit, cn = dit.to(BF).cuda(), cn.to(BF).cuda()
    for p_ in dit.parameters():
        p_.requires_grad_(False)
    pipe = WanVideoPipeline.from_modules(dit, None, cn, None, device="cuda")
    pipe.scheduler.set_timesteps(1000, training=True)
    dev = {k: v.cuda() for k, v in inp.items()}
    loss = pipe.training_loss(input_latents=dev["input_latents"], noise=dev["noise"], context=dev["context"], y=dev["y"],
                              control_signal_video_latents=dev["control"], timestep_id=tid)
    loss.backward()
    named = dict(cn.named_parameters())
    assert sorted(named) == sorted(g_ref) and all(p_.grad is None for p_ in dit.parameters())
    got = {n: named[n].grad.cpu() for n in g_ref}
    lv = float(loss.detach())
    print(f"LOSS device {lv:.7f} fp64 {loss_ref:.7f} restatement {l0:.7f}: {abs(lv - loss_ref) / abs(l0 - loss_ref):.3f} of its distance (bar {T.LOSS_MARGIN})")
    if zero:
        for n, t in got.items():
            if "zero_convs" not in n:
                assert not bool(t.any()), f"{n}: behind zero convs every ControlNet gradient is exactly zero"
    T.assert_rows(got, c0, g_ref, f"whole tape zero_convs_zero={zero}", model=True)
    assert abs(lv - loss_ref) <= T.LOSS_MARGIN * abs(l0 - loss_ref), (lv, loss_ref, l0)
