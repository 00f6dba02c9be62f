"""The row and elementwise training kernels of gf_backward.hip against fp64 references, at every dispatch path and width.

Every bf16 gradient is held, element by element, to  |got - ref| <= 2^-8 |ref| + 2^-16 scale  (tests/backward_refs.py: half a bf16 ulp of
the exact value plus ~128 fp32 epsilons of the quantity's natural magnitude); tests/test_backward_refs_cpu.py shows on the CPU that an fp32
restatement of each kernel is inside that bound and that a row mean missing ONE 16-byte chunk at dim = 5120 is outside it (the 6e-3 rel-L2
bar used before lets that through).  fp32 results keep the project's bars: column sums, loss, sumsq 1e-5; the xhat-weighted sums dg / dw
2e-3; AdamW's moments 1e-5 / 1e-4.

Paths (gf_layernorm_bwd and gf_rmsnorm_rope_bwd alike):  no accumulator and dim <= 5120 -> the wave-per-row kernel (10 chunk slots of 8
columns per lane: 512 fills slot 0, 520 starts slot 1, 5112 leaves the last lane's tenth slot empty, 5120 fills all);  an accumulator -> the
block kernel (16 rows per workgroup, 8 chunk slots per thread: 1024 / 1032 / 8192 likewise, atomic column sums);  no accumulator and
dim > 5120 -> the block kernel again.

The tests print what they measure (`pytest -s`): lines `FLOOR` give the worst per-row rel-L2 of dx over the bf16 rounding floor
rel_l2(ref.to(bf16), ref) at dim 5120 for both kernels (the CPU restatement: 1.000), `COLSUM` / `MANY` the accumulators' rel-L2, `LOSS` and
`SUMSQ` the relative errors of the scalars, `ADAMW` the moments' rel-L2 and the parameter's worst share of its allowance.
"""
import pytest
import torch

import backward_refs as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DIMS = (8, 256, 512, 520, 1024, 1032, 1536, 5112, 5120, 5128, 8192)      # wave, block and fallback dims of both row operations
ROWS = (1, 9, 17, 37)       # 9: a partial last workgroup of the wave kernels (8 rows each); 17: of the block kernels (16 rows each)
SENTINEL = 0x5A5A           # a finite bf16 bit pattern no kernel here produces by accident in a whole margin


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from goal_force_amd import ops as _ops
    return _ops


@pytest.fixture
def no_launch(ops, monkeypatch):
    """Inside this fixture a call that gets as far as the library fails the test instead of launching: the argument mistakes below must be
    stopped by ops.py itself, before a kernel could read or write past a buffer."""
    def reached():
        raise AssertionError("the call reached the HIP library: ops.py did not refuse it")
    monkeypatch.setattr(ops._lib, "load", reached)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _c(t):
    return None if t is None else t.cuda()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _acc(dim, init):
    return torch.zeros(dim, device="cuda") if init is None else init.clone().cuda()


def _check_acc(acc, init, ref, bar, what):
    want = ref if init is None else ref + init.double()
    e = R.rel_l2(acc.cpu(), want)
    print(f"{what}: rel-L2 {e:.3e} (bar {bar:g})")
    assert e <= bar, f"{what}: rel-L2 {e:.3e} > {bar:g}"
    return e


def _hds(dim):
    return [h for h in (128, 64) if dim % h == 0] or [8]


# ---------------------------------------------------------------------------------------------------------------------
# B1 LayerNorm backward
def _ln_inputs(rows, dim, gmode, seed):
    x, dy, g = R.row_inputs(rows, dim, _gen(seed), gmode)
    if rows >= 37:
        x[5] = 2.5                                                      # a constant row: variance 0, rstd = eps^-1/2
    return x, dy, g


@pytest.mark.parametrize("gmode", ["none", "affine", "scale1p"])
@pytest.mark.parametrize("dim", DIMS)
def test_layernorm_bwd_every_path(ops, dim, gmode):
    """Without accumulators (wave kernel; block kernel above 5120) and with both (block kernel) on the same inputs."""
    for rows in ROWS:
        x, dy, g = _ln_inputs(rows, dim, gmode, 1000 * rows + dim)
        dx_ref, dg_ref, db_ref = R.layernorm_bwd_ref(x, dy, g)
        scale = R.row_rms(dx_ref)
        what = f"layernorm_bwd ({rows}, {dim}) g={gmode}"
        dx = ops.layernorm_bwd(_c(x), _c(dy), g=_c(g))
        assert dx.dtype == BF and dx.shape == x.shape
        R.assert_within(dx.cpu(), dx_ref, scale, what + " no accumulators")
        dg, db = _acc(dim, None), _acc(dim, None)
        dx2 = ops.layernorm_bwd(_c(x), _c(dy), g=_c(g), dg_acc=dg, db_acc=db)
        R.assert_within(dx2.cpu(), dx_ref, scale, what + " dg+db")
        _check_acc(dg, None, dg_ref, 2e-3, what + " dg")
        _check_acc(db, None, db_ref, 1e-5, what + " db")
        if dim == 5120:
            print(f"FLOOR {what}: dx/floor wave {R.floor_ratio(dx.cpu(), dx_ref):.4f} block {R.floor_ratio(dx2.cpu(), dx_ref):.4f}")


@pytest.mark.parametrize("rows,dim", [(17, 1536), (37, 5120)])
def test_layernorm_bwd_one_accumulator_and_nonzero_start(ops, rows, dim):
    x, dy, g = _ln_inputs(rows, dim, "scale1p", 5)
    dx_ref, dg_ref, db_ref = R.layernorm_bwd_ref(x, dy, g)
    both = ops.layernorm_bwd(_c(x), _c(dy), g=_c(g), dg_acc=_acc(dim, None), db_acc=_acc(dim, None))
    R.assert_within(both.cpu(), dx_ref, R.row_rms(dx_ref), "dx")
    init_g, init_b = torch.randn(dim, generator=_gen(6)), 3 * torch.randn(dim, generator=_gen(7))
    for ig, ib in ((None, None), (init_g, init_b)):
        dg = _acc(dim, ig)
        dx = ops.layernorm_bwd(_c(x), _c(dy), g=_c(g), dg_acc=dg)
        assert torch.equal(_bits(dx), _bits(both)), "dg only: dx must not depend on which sums are wanted"
        _check_acc(dg, ig, dg_ref, 2e-3, f"dg alone, start {'zero' if ig is None else 'non-zero'}")
        db = _acc(dim, ib)
        dx = ops.layernorm_bwd(_c(x), _c(dy), g=_c(g), db_acc=db)
        assert torch.equal(_bits(dx), _bits(both))
        _check_acc(db, ib, db_ref, 1e-5, f"db alone, start {'zero' if ib is None else 'non-zero'}")
        dg, db = _acc(dim, ig), _acc(dim, ib)
        ops.layernorm_bwd(_c(x), _c(dy), g=_c(g), dg_acc=dg, db_acc=db)
        _check_acc(dg, ig, dg_ref, 2e-3, "dg of both")
        _check_acc(db, ib, db_ref, 1e-5, "db of both")


@pytest.mark.parametrize("rows,dim", [(4100, 1536), (2051, 5120)])
def test_layernorm_bwd_many_workgroups_on_the_atomics(ops, rows, dim):
    x, dy, g = _ln_inputs(rows, dim, "affine", 8)
    dx_ref, dg_ref, db_ref = R.layernorm_bwd_ref(x, dy, g)
    dg, db = _acc(dim, None), _acc(dim, None)
    dx = ops.layernorm_bwd(_c(x), _c(dy), g=_c(g), dg_acc=dg, db_acc=db)
    R.assert_within(dx.cpu(), dx_ref, R.row_rms(dx_ref), f"layernorm_bwd ({rows}, {dim}) dx")
    _check_acc(dg, None, dg_ref, 2e-3, f"MANY layernorm_bwd ({rows}, {dim}) dg")
    _check_acc(db, None, db_ref, 1e-5, f"MANY layernorm_bwd ({rows}, {dim}) db")


# ---------------------------------------------------------------------------------------------------------------------
# B2 RMSNorm(+RoPE) backward
def _rms_inputs(rows, dim, seed):
    x, dy, w = R.row_inputs(rows, dim, _gen(seed), "affine")
    if rows >= 37:
        x[7] = 0.0                                                      # an all-zero row: rstd = eps^-1/2, xn = 0
    return x, dy, w


def _rms_both_kernels(ops, x, dy, w, cos, sin, hd, what):
    rows, dim = x.shape
    dx_ref, dw_ref = R.rmsnorm_rope_bwd_ref(x, dy, w, cos, sin, hd)
    scale = R.row_rms(dx_ref)
    dx = ops.rmsnorm_rope_bwd(_c(x), _c(dy), _c(w), _c(cos), _c(sin), hd, 1e-6)
    assert dx.dtype == BF and dx.shape == x.shape
    R.assert_within(dx.cpu(), dx_ref, scale, what + " no accumulator")
    dw = _acc(dim, None)
    dx2 = ops.rmsnorm_rope_bwd(_c(x), _c(dy), _c(w), _c(cos), _c(sin), hd, 1e-6, dw_acc=dw)
    R.assert_within(dx2.cpu(), dx_ref, scale, what + " dw")
    _check_acc(dw, None, dw_ref, 2e-3, what + " dw")
    if dim == 5120:
        print(f"FLOOR {what}: dx/floor wave {R.floor_ratio(dx.cpu(), dx_ref):.4f} block {R.floor_ratio(dx2.cpu(), dx_ref):.4f}")
    return dx_ref, dw_ref


@pytest.mark.parametrize("dim", DIMS)
def test_rmsnorm_rope_bwd_every_path(ops, dim):
    """Without dw_acc (wave kernel; block kernel above 5120) and with it (block kernel), with and without RoPE, at each head_dim."""
    for rows in ROWS:
        x, dy, w = _rms_inputs(rows, dim, 2000 * rows + dim)
        hds = _hds(dim)
        _rms_both_kernels(ops, x, dy, w, None, None, hds[0], f"rmsnorm_bwd ({rows}, {dim})")
        for hd in hds:
            cos, sin = R.rope_table(rows, hd, _gen(rows + hd))
            _rms_both_kernels(ops, x, dy, w, cos, sin, hd, f"rmsnorm_rope_bwd ({rows}, {dim}) head_dim={hd}")


def test_rmsnorm_rope_bwd_is_the_transpose_for_a_prescaled_table(ops):
    """The q side of self-attention passes the table times Q_PRESCALE(128) (the softmax scale and log2 e folded into q): not a rotation any
    more, and the backward must still be the transpose of the forward map."""
    from goal_force_amd.dit import Q_PRESCALE
    rows, dim, hd = 37, 5120, 128
    x, dy, w = _rms_inputs(rows, dim, 9)
    cos, sin = R.rope_table(rows, hd, _gen(10), Q_PRESCALE(hd))
    _rms_both_kernels(ops, x, dy, w, cos, sin, hd, "rmsnorm_rope_bwd prescaled table")
    # a table longer than the rows (the whole sequence's table with a shorter x) is fine: rows index it from the start
    cos2, sin2 = torch.cat([cos, cos]), torch.cat([sin, sin])
    a = ops.rmsnorm_rope_bwd(_c(x), _c(dy), _c(w), _c(cos), _c(sin), hd, 1e-6)
    b = ops.rmsnorm_rope_bwd(_c(x), _c(dy), _c(w), _c(cos2), _c(sin2), hd, 1e-6)
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("rows,dim", [(4100, 1536), (2051, 5120)])
def test_rmsnorm_rope_bwd_many_workgroups_on_the_atomics(ops, rows, dim):
    x, dy, w = _rms_inputs(rows, dim, 11)
    cos, sin = R.rope_table(rows, 128, _gen(12))
    dx_ref, dw_ref = R.rmsnorm_rope_bwd_ref(x, dy, w, cos, sin, 128)
    init = torch.randn(dim, generator=_gen(13))
    dw = _acc(dim, init)
    dx = ops.rmsnorm_rope_bwd(_c(x), _c(dy), _c(w), _c(cos), _c(sin), 128, 1e-6, dw_acc=dw)
    R.assert_within(dx.cpu(), dx_ref, R.row_rms(dx_ref), f"rmsnorm_rope_bwd ({rows}, {dim}) dx")
    _check_acc(dw, init, dw_ref, 2e-3, f"MANY rmsnorm_rope_bwd ({rows}, {dim}) dw, non-zero start")


# ---------------------------------------------------------------------------------------------------------------------
# B3 row strides and out-of-bounds writes, through the C ABI
def _strided_operands(rows, dim, seed):
    """x and dy as column slices of wider buffers (two different strides); dx as a column slice of a sentinel-filled buffer with margins
    left, right and below."""
    g = _gen(seed)
    xw = (torch.randn((rows, dim + 24), generator=g) * 1.5 + 0.3).to(BF).cuda()
    dyw = torch.randn((rows, dim + 64), generator=g).to(BF).cuda()
    buf = torch.full((rows + 3, dim + 40), SENTINEL, dtype=torch.int16, device="cuda").view(BF)
    return xw[:, 8:8 + dim], dyw[:, 48:48 + dim], buf, buf[:rows, 16:16 + dim]


def _check_sentinels(buf, view, want, what):
    rows, dim = view.shape
    torch.cuda.synchronize()
    assert torch.equal(_bits(view), _bits(want)), f"{what}: strided call differs from the contiguous one"
    margins = buf.view(torch.int16).clone()
    margins[:rows, 16:16 + dim] = SENTINEL
    assert bool((margins == SENTINEL).all()), f"{what}: wrote outside dx ({int((margins != SENTINEL).sum())} elements)"


@pytest.mark.parametrize("rows,dim,acc", [(9, 520, False), (9, 5120, False), (17, 1032, True), (17, 5120, True), (9, 5128, False)])
def test_layernorm_bwd_row_strides_and_margins(ops, rows, dim, acc):
    from goal_force_amd import _lib
    x, dy, buf, dxv = _strided_operands(rows, dim, dim + rows)
    g = (1 + 0.2 * torch.randn(dim, generator=_gen(1))).to(BF).cuda()
    assert x.stride(0) != dy.stride(0) != dxv.stride(0) and not x.is_contiguous()
    dg, db = (_acc(dim, None), _acc(dim, None)) if acc else (None, None)
    want = ops.layernorm_bwd(x.contiguous(), dy.contiguous(), g=g, dg_acc=None if not acc else _acc(dim, None),
                             db_acc=None if not acc else _acc(dim, None))
    st = torch.cuda.current_stream().cuda_stream
    rc = _lib.load().gf_layernorm_bwd(x.data_ptr(), x.stride(0), dy.data_ptr(), dy.stride(0), g.data_ptr(), dxv.data_ptr(), dxv.stride(0),
                                      None if dg is None else dg.data_ptr(), None if db is None else db.data_ptr(), rows, dim, 1e-6, st)
    assert rc == 0
    _check_sentinels(buf, dxv, want, f"gf_layernorm_bwd ({rows}, {dim}) acc={acc}")
    dx_ref, dg_ref, db_ref = R.layernorm_bwd_ref(x.cpu(), dy.cpu(), g.cpu())
    R.assert_within(dxv.cpu(), dx_ref, R.row_rms(dx_ref), "strided dx")
    if acc:
        _check_acc(dg, None, dg_ref, 2e-3, "strided dg")
        _check_acc(db, None, db_ref, 1e-5, "strided db")
    # the wrapper passes x's and dy's strides on: the same bits
    assert torch.equal(_bits(ops.layernorm_bwd(x, dy, g=g, dg_acc=None if not acc else _acc(dim, None))), _bits(want))


@pytest.mark.parametrize("rows,dim,hd,acc", [(9, 520, 8, False), (9, 5120, 128, False), (17, 1032, 8, True), (17, 5120, 128, True),
                                             (9, 5128, 8, False)])
def test_rmsnorm_rope_bwd_row_strides_and_margins(ops, rows, dim, hd, acc):
    from goal_force_amd import _lib
    x, dy, buf, dxv = _strided_operands(rows, dim, dim + rows + 1)
    w = (1 + 0.2 * torch.randn(dim, generator=_gen(2))).to(BF).cuda()
    cos, sin = (t.cuda() for t in R.rope_table(rows, hd, _gen(3)))
    dw = _acc(dim, None) if acc else None
    want = ops.rmsnorm_rope_bwd(x.contiguous(), dy.contiguous(), w, cos, sin, hd, 1e-6, dw_acc=_acc(dim, None) if acc else None)
    st = torch.cuda.current_stream().cuda_stream
    rc = _lib.load().gf_rmsnorm_rope_bwd(x.data_ptr(), x.stride(0), dy.data_ptr(), dy.stride(0), w.data_ptr(), cos.data_ptr(), sin.data_ptr(),
                                         dxv.data_ptr(), dxv.stride(0), None if dw is None else dw.data_ptr(), rows, dim, hd, 1e-6, st)
    assert rc == 0
    _check_sentinels(buf, dxv, want, f"gf_rmsnorm_rope_bwd ({rows}, {dim}) acc={acc}")
    dx_ref, dw_ref = R.rmsnorm_rope_bwd_ref(x.cpu(), dy.cpu(), w.cpu(), cos.cpu(), sin.cpu(), hd)
    R.assert_within(dxv.cpu(), dx_ref, R.row_rms(dx_ref), "strided dx")
    if acc:
        _check_acc(dw, None, dw_ref, 2e-3, "strided dw")
    assert torch.equal(_bits(ops.rmsnorm_rope_bwd(x, dy, w, cos, sin, hd, 1e-6, dw_acc=_acc(dim, None) if acc else None)), _bits(want))


# ---------------------------------------------------------------------------------------------------------------------
# B4 what the C ABI refuses (each returns before any launch; every buffer is large enough for the call as made all the same)
def test_row_backward_c_abi_refusals(ops):
    from goal_force_amd import _lib
    from goal_force_amd._lib import GoalForceError
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    rows = 4
    big = lambda: torch.zeros((rows, 8256), dtype=BF, device="cuda")      # noqa: E731
    x, dy, dx, vec = big(), big(), big(), torch.ones(8256, dtype=BF, device="cuda")
    tab = torch.ones(rows * 4128, dtype=torch.float32, device="cuda")
    p = lambda t: t.data_ptr()                                            # noqa: E731

    def ln(dim, xs=8256, dys=8256, dxs=8256):
        return lib.gf_layernorm_bwd(p(x), xs, p(dy), dys, p(vec), p(dx), dxs, None, None, rows, dim, 1e-6, st)

    def rms(dim, hd=8, cos=tab, sin=tab, xs=8256, dys=8256, dxs=8256):
        return lib.gf_rmsnorm_rope_bwd(p(x), xs, p(dy), dys, p(vec), None if cos is None else p(cos), None if sin is None else p(sin),
                                       p(dx), dxs, None, rows, dim, hd, 1e-6, st)

    assert ln(8192) == 0 and rms(8192) == 0 and rms(256, 128, None, None) == 0      # the same calls with arguments the ABI accepts
    refused = {"layernorm dim 8200": lambda: ln(8200), "layernorm dim 260": lambda: ln(260),
               "layernorm x stride 8260": lambda: ln(512, xs=8260), "layernorm dy stride 8260": lambda: ln(512, dys=8260),
               "layernorm dx stride 8252": lambda: ln(512, dxs=8252),
               "rmsnorm dim 8200": lambda: rms(8200), "rmsnorm dim 260": lambda: rms(260, 4),
               "rmsnorm head_dim 48 of dim 256": lambda: rms(256, 48), "rmsnorm head_dim 12": lambda: rms(240, 12),
               "rmsnorm cos without sin": lambda: rms(256, 128, tab, None), "rmsnorm sin without cos": lambda: rms(256, 128, None, tab),
               "rmsnorm x stride 8260": lambda: rms(512, xs=8260), "rmsnorm dx stride 8252": lambda: rms(512, dxs=8252)}
    for what, call in refused.items():
        with pytest.raises(GoalForceError):
            _lib.check(call(), what)
    torch.cuda.synchronize()
    xb = torch.zeros((rows, 8200), dtype=BF, device="cuda")
    for bad in (xb, xb[:, :260]):
        with pytest.raises(GoalForceError):
            ops.layernorm_bwd(bad, bad)
        with pytest.raises(GoalForceError):
            ops.rmsnorm_rope_bwd(bad, bad, vec[:bad.shape[1]].contiguous(), head_dim=8)


# ---------------------------------------------------------------------------------------------------------------------
# C what ops.py refuses before the library is reached
def test_layernorm_bwd_wrapper_refuses_mismatched_shapes(ops, no_launch):
    from goal_force_amd._lib import GoalForceError
    rows, dim = 9, 512
    x = torch.zeros((rows, dim), dtype=BF, device="cuda")
    vec = lambda n, dt=BF: torch.zeros(n, dtype=dt, device="cuda")        # noqa: E731
    f32 = torch.float32
    bad = [dict(dy=x[:-1]), dict(dy=torch.zeros((rows + 1, dim), dtype=BF, device="cuda")), dict(dy=x[:, :dim - 8]),
           dict(dy=torch.zeros((rows, dim + 8), dtype=BF, device="cuda")), dict(dy=x.float()), dict(dy=x.cpu()),
           dict(g=vec(dim - 8)), dict(g=vec(2 * dim)), dict(g=vec(2 * dim)[::2]), dict(g=vec(dim, f32)),
           dict(dg_acc=vec(dim - 8, f32)), dict(dg_acc=vec(dim + 8, f32)), dict(dg_acc=vec(dim)), dict(dg_acc=vec(2 * dim, f32)[::2]),
           dict(db_acc=vec(dim - 8, f32)), dict(db_acc=vec(1, f32)), dict(db_acc=vec(dim, torch.float64))]
    for kw in bad:
        with pytest.raises(GoalForceError):
            ops.layernorm_bwd(x, kw.pop("dy", x), **kw)


def test_rmsnorm_rope_bwd_wrapper_refuses_mismatched_shapes(ops, no_launch):
    from goal_force_amd._lib import GoalForceError
    rows, dim, hd = 9, 512, 128
    x = torch.zeros((rows, dim), dtype=BF, device="cuda")
    w = torch.ones(dim, dtype=BF, device="cuda")
    tab = lambda n: torch.ones(n, dtype=torch.float32, device="cuda")      # noqa: E731
    ok = tab(rows * hd // 2)
    bad = [dict(dy=x[:-1]), dict(dy=x[:, :dim - 8]), dict(weight=w[:dim - 8]), dict(weight=torch.ones(dim + 8, dtype=BF, device="cuda")),
           dict(weight=None), dict(weight=w.float()),
           dict(cos=ok), dict(sin=ok), dict(cos=tab(rows * hd // 2 - 4), sin=ok), dict(cos=ok, sin=tab(rows * hd // 2 - 4)),
           dict(cos=tab((rows - 1) * hd // 2), sin=tab((rows - 1) * hd // 2)), dict(cos=ok.to(BF), sin=ok.to(BF)),
           dict(cos=tab(rows * hd)[::2], sin=ok), dict(cos=tab(rows * 32), sin=tab(rows * 32)),          # a table for head_dim 64
           dict(head_dim=48), dict(head_dim=0), dict(head_dim=4),
           dict(dw_acc=tab(dim - 8)), dict(dw_acc=tab(dim + 8)), dict(dw_acc=torch.zeros(dim, dtype=BF, device="cuda"))]
    for kw in bad:
        with pytest.raises(GoalForceError):
            ops.rmsnorm_rope_bwd(x, kw.pop("dy", x), kw.pop("weight", w), **{"head_dim": hd, **kw})


def test_colsum_wrapper_refuses_mismatched_shapes(ops, no_launch):
    from goal_force_amd._lib import GoalForceError
    rows, cols = 9, 512
    a = torch.zeros((rows, cols), dtype=BF, device="cuda")
    f = lambda n: torch.zeros(n, dtype=torch.float32, device="cuda")       # noqa: E731
    v = lambda n: torch.zeros(n, dtype=BF, device="cuda")                  # noqa: E731
    bad = [dict(b=a[:-1], acc=f(cols)), dict(b=a[:, :cols - 8], acc=f(cols)), dict(b=torch.zeros((rows + 1, cols), dtype=BF, device="cuda"), acc=f(cols)),
           dict(b=a.float(), acc=f(cols)), dict(gate=v(cols - 8)), dict(gate=v(cols + 8)), dict(gate=v(2 * cols)[::2]), dict(gate=f(cols)),
           dict(acc=f(cols - 8)), dict(acc=f(cols + 8)), dict(acc=v(cols)), dict(acc=f(2 * cols)[::2]), dict(gate=v(cols), acc=f(cols - 8)),
           dict()]
    for kw in bad:
        with pytest.raises(GoalForceError):
            ops.colsum(a, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# B5 colsum
@pytest.mark.parametrize("rows,cols", [(1, 8), (63, 512), (64, 2048), (65, 2056), (130, 5120), (65, 13824), (4100, 512), (4100, 2056)])
def test_colsum_four_modes(ops, rows, cols):
    g = _gen(rows * 3 + cols)
    a, b = torch.randn((rows, cols), generator=g).to(BF), torch.randn((rows, cols), generator=g).to(BF)
    gate = torch.randn((cols,), generator=g).to(BF)
    init = torch.randn(cols, generator=g)
    ac, bc, gc = _c(a), _c(b), _c(gate)
    what = f"COLSUM ({rows}, {cols})"
    for start in (None, init):
        acc = _acc(cols, start)
        assert ops.colsum(ac, acc=acc) is None
        _check_acc(acc, start, R.colsum_ref(a), 1e-5, what + " acc")
        acc = _acc(cols, start)
        assert ops.colsum(ac, b=bc, acc=acc) is None
        _check_acc(acc, start, R.colsum_ref(a, b), 1e-5, what + " acc + b")
        acc = _acc(cols, start)
        out = ops.colsum(ac, b=bc, gate=gc, acc=acc)
        _check_acc(acc, start, R.colsum_ref(a, b), 1e-5, what + " acc + b + gate")
        assert out.dtype == BF and torch.equal(_bits(out.cpu()), _bits(R.gated_ref(a, gate)))
    out = ops.colsum(ac, gate=gc)                                      # gate only: what the block's forward issues for x + gate * o
    assert torch.equal(_bits(out.cpu()), _bits(R.gated_ref(a, gate)))


@pytest.mark.parametrize("rows,cols", [(65, 2056), (130, 520)])
def test_colsum_column_slices_with_their_own_leading_dimensions(ops, rows, cols):
    g = _gen(rows + cols)
    aw, bw = torch.randn((rows, cols + 24), generator=g).to(BF).cuda(), torch.randn((rows, 2 * cols + 8), generator=g).to(BF).cuda()
    a, b = aw[:, 16:16 + cols], bw[:, cols:2 * cols]
    gate = torch.randn((cols,), generator=g).to(BF).cuda()
    assert a.stride(0) != b.stride(0) and not a.is_contiguous()
    acc = _acc(cols, None)
    out = ops.colsum(a, b=b, gate=gate, acc=acc)
    _check_acc(acc, None, R.colsum_ref(a.cpu(), b.cpu()), 1e-5, f"COLSUM strided ({rows}, {cols})")
    assert out.is_contiguous() and torch.equal(_bits(out.cpu()), _bits(R.gated_ref(a.cpu(), gate.cpu())))
    assert torch.equal(_bits(ops.colsum(a, gate=gate)), _bits(out))
    acc = _acc(cols, None)
    ops.colsum(a, acc=acc)
    _check_acc(acc, None, R.colsum_ref(a.cpu()), 1e-5, "COLSUM strided a alone")


# ---------------------------------------------------------------------------------------------------------------------
# B6 act_bwd
@pytest.mark.parametrize("n", [8, 4104, 66560])
@pytest.mark.parametrize("kind", ["gelu_tanh", "silu"])
def test_act_bwd(ops, kind, n):
    u, df = R.act_inputs(n, _gen(n))
    ref = R.act_bwd_ref(u, df, kind)
    got = ops.act_bwd(_c(u), _c(df), kind).cpu()
    assert bool(torch.isfinite(got.float())[torch.isfinite(ref)].all()), "non-finite where the derivative is finite"
    R.assert_within(got, ref, df.double().abs(), f"act_bwd {kind} n={n}")


# ---------------------------------------------------------------------------------------------------------------------
# B7 mse_loss
@pytest.mark.parametrize("weight", [1.0, 0.37])
@pytest.mark.parametrize("n", [8, 1003, 300007])
def test_mse_loss(ops, n, weight):
    """300 007 > 1024 blocks x 256: the grid-stride loop iterates and ends on a ragged tail."""
    g = _gen(n)
    p, t = torch.randn((n,), generator=g).to(BF), torch.randn((n,), generator=g).to(BF)
    loss_ref, grad_ref = R.mse_ref(p, t, weight)
    loss, grad = ops.mse_loss(_c(p), _c(t), weight=weight)
    e = abs(float(loss) - loss_ref) / loss_ref
    print(f"LOSS mse n={n} weight={weight}: relative error {e:.3e}")
    assert loss.dtype == torch.float32 and loss.shape == (1,) and e <= 1e-5
    R.assert_within(grad.cpu(), grad_ref, grad_ref.abs(), f"mse gradient n={n} weight={weight}")
    loss2, none = ops.mse_loss(_c(p), _c(t), weight=weight, want_grad=False)
    assert none is None
    same = torch.equal(loss2.view(torch.int32), loss.view(torch.int32))
    print(f"LOSS mse n={n} weight={weight}: want_grad=False gives {float(loss2)!r}, want_grad=True {float(loss)!r}, same bits: {same}")
    assert same, "the loss must not depend on want_grad"
    zero, gz = ops.mse_loss(_c(p), _c(p.clone()), weight=weight)
    assert float(zero) == 0.0 and not bool(gz.float().any())


# ---------------------------------------------------------------------------------------------------------------------
# B8 sumsq
@pytest.mark.parametrize("n", [1, 1003, 600011])
def test_sumsq(ops, n):
    """600 011 > 2048 blocks x 256: the grid-stride loop iterates."""
    x = torch.randn((n,), generator=_gen(n)).to(BF)
    ref = R.sumsq_ref(x)
    acc = torch.zeros(1, device="cuda")
    ops.sumsq(_c(x), acc)
    e1 = abs(float(acc) - ref) / ref
    ops.sumsq(_c(x), acc)                                               # a second call adds
    e2 = abs(float(acc) - 2 * ref) / (2 * ref)
    print(f"SUMSQ n={n}: relative error {e1:.3e}, after a second call {e2:.3e}")
    assert e1 <= 1e-5 and e2 <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# B9 f32_to_bf16
def _f32_to_bf16_inputs(n, g):
    """n fp32 values: specials first (n >= 12), then thirds of exact ties, values one fp32 ulp off a tie, and random magnitudes."""
    k = max(1, -(-(n - 12) // 3))
    hi = torch.randint(0x0080, 0x7F00, (k,), generator=g, dtype=torch.int32)           # normal, finite upper halves, even and odd
    sgn = torch.randint(0, 2, (k,), generator=g).float() * 2 - 1
    ties = ((hi << 16) | 0x8000).view(torch.float32) * sgn                             # exactly half way: up for odd, down for even
    near = ((hi << 16) | (0x7FFF + 2 * (hi % 2 == 0).int())).view(torch.float32) * sgn     # 0x8001 after even, 0x7FFF after odd
    x = torch.randn((k,), generator=g) * torch.pow(10.0, torch.randint(-20, 20, (k,), generator=g).float())
    if n < 12:
        return torch.cat([ties, near, x])[:n]
    fmax = torch.finfo(torch.float32).max
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), fmax, -fmax, float("nan"), 1.0, -1.0, 2.0 ** -126])
    nan_low = torch.tensor([0x7F800001, 0x7FC00000], dtype=torch.int32).view(torch.float32)   # a NaN whose payload sits in the low half
    return torch.cat([special, nan_low, ties, near, x])[:n]


@pytest.mark.parametrize("n", [1, 1003, 30720])
def test_f32_to_bf16_is_round_to_nearest_even(ops, n):
    src = _f32_to_bf16_inputs(n, _gen(n))
    assert src.numel() == n
    got = ops.f32_to_bf16(_c(src)).cpu()
    want = src.to(BF)
    assert got.dtype == BF and got.shape == src.shape
    nan = torch.isnan(src)
    assert bool(torch.isnan(got.float())[nan].all()), "NaN must stay NaN"
    assert torch.equal(_bits(got)[~nan], _bits(want)[~nan])
    if n >= 12:
        assert int(nan.sum()) == 3 and bool(torch.isinf(got.float()[2:6]).all()), "the largest finite fp32 rounds to inf"


def test_f32_to_bf16_keeps_the_shape_and_ties_go_both_ways(ops):
    src = torch.tensor([[0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001]], dtype=torch.int32).view(torch.float32)
    got = ops.f32_to_bf16(_c(src)).cpu()
    assert got.shape == (1, 4)
    assert _bits(got).tolist() == [[0x3F80, 0x3F82, 0x3F80, 0x3F81]]    # tie to even (down), tie to even (up), below, above


# ---------------------------------------------------------------------------------------------------------------------
# B10 AdamW
@pytest.mark.parametrize("case", R.ADAMW_CASES, ids=R.adamw_id)
def test_adamw_one_step_from_given_state(ops, case):
    """The moments are where a wrong grad_scale shows (linear in m, quadratic in v): the parameter update m / sqrt(v) hardly moves with it."""
    kw = {k: v for k, v in case.items() if k != "moments"}
    n = 1003
    p, gr, m, v = R.adamw_state(n, case["moments"], 7)
    ref = R.adamw_ref(p, gr, m, v, lr=1e-2, **kw)
    pc, mc, vc = _c(p.clone()), _c(m.clone()), _c(v.clone())
    ver = pc._version
    ops.adamw_step(pc, _c(gr), mc, vc, lr=1e-2, **kw)
    assert pc._version > ver, "adamw_step writes through the raw pointer and must tell torch"
    R.adamw_check(pc.cpu(), mc.cpu(), vc.cpu(), ref, f"ADAMW {R.adamw_id(case)}")
