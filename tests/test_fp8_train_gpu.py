"""Training through frozen fp8 blocks on the device: gf_quant_fp8_grad and gf_cast_fp8_t through the raw C ABI bit for bit against
their restatements, training.linear_dx_fp8 against the exact chain on the device's own codes through gemm_refs' two fp8 bars, the frozen
fp8 block's tape and the ControlNet step over an fp8-frozen expert through the row statistic with the bars of tests/fp8_train_refs.py
(measured on the CPU by tests/test_fp8_train_cpu.py, none read off the device).  `pytest -s` prints every figure (`PIN`, `ROW`, `LOSS`)."""
import functools
import importlib.util
import math
import os

import pytest
import torch

import fp8_train_refs as F
import gemm_refs as GR
import tape_refs as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
NAN_BITS = 0x7FC1                 # a quiet-NaN bf16 pattern no kernel writes (as int16)
FILL8 = 0xA5                      # what a byte destination holds before a call (the quantiser's strided parent: 0xFF)
GUARD = 96


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from goal_force_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _state():
    """Autograd on (other modules switch it off process-wide); the fp8 switch off before and restored after every test."""
    from goal_force_amd import training
    old = training.set_fp8_frozen(False)
    with torch.enable_grad():
        yield
    training.set_fp8_frozen(old)


def _lib(ops):
    return ops._lib.load()


def _err(ops):
    return _lib(ops).gf_last_error().decode("utf-8", "replace")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_scales(got, want):
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))


# ---------------------------------------------------------------------------------------------------------------------
# a. gf_quant_fp8_grad, raw C ABI
def _quant_call(ops, x, x_extra=0, out_extra=0):
    """x [rows, dim] bf16 (CPU) laid into a NaN parent with row pitch dim + x_extra, quantised into a 0xFF parent with row pitch
    dim + out_extra, the scales between sentinels -> (rc, codes [rows, dim], scales [rows]); everything around must be untouched."""
    rows, dim = x.shape
    xs, os_ = dim + x_extra, dim + out_extra
    src = torch.full((rows * xs + 8,), NAN_BITS, dtype=torch.int16)
    src[:rows * xs].view(rows, xs)[:, :dim] = x.view(torch.int16)
    dst = torch.full((GUARD + rows * os_ + GUARD,), 0xFF, dtype=torch.uint8)
    sc = torch.full((4 + rows + 4,), -7.5, dtype=torch.float32)
    psrc, pdst, psc = src.cuda(), dst.cuda(), sc.cuda()
    rc = _lib(ops).gf_quant_fp8_grad(psrc.data_ptr(), pdst.data_ptr() + GUARD, psc.data_ptr() + 16, rows, dim, xs, os_, _st())
    out, s = pdst.cpu(), psc.cpu()
    what = f"quant_fp8_grad rows={rows} dim={dim} x pitch {xs} out pitch {os_}"
    assert bool((out[:GUARD] == 0xFF).all()) and bool((out[GUARD + rows * os_:] == 0xFF).all()), f"{what}: a byte around out8 was written"
    body = out[GUARD:GUARD + rows * os_].view(rows, os_)
    assert bool((body[:, dim:] == 0xFF).all()), f"{what}: the gap behind a row of out8 was written"
    assert bool((s[:4] == -7.5).all()) and bool((s[4 + rows:] == -7.5).all()), f"{what}: a sentinel beside scale was written"
    return rc, body[:, :dim].contiguous(), s[4:4 + rows].clone(), what


def _assert_quant(ops, x, **kw):
    rc, codes, scale, what = _quant_call(ops, x, **kw)
    assert rc == 0, f"{what}: {_err(ops)}"
    want_c, want_s = F.quant_grad_ref(x)
    assert _same_scales(scale, want_s), f"{what}: scales differ at rows {torch.nonzero(~(scale == want_s) & ~(torch.isnan(scale) & torch.isnan(want_s))).flatten()[:4].tolist()}"
    assert torch.equal(codes, want_c), f"{what}: codes differ at {torch.nonzero(codes != want_c)[:4].tolist()}"


QUANT_DIMS = (8, 136, 256, 512, 5120, 13824, 14336)
QUANT_ROWS = (1, 3, 4, 5, 65)


@pytest.mark.parametrize("dim", QUANT_DIMS)
def test_quant_fp8_grad_bit_for_bit(ops, dim):
    for rows in QUANT_ROWS:
        _assert_quant(ops, F.gauss_rows(rows, dim, seed=1))
    _assert_quant(ops, F.hand_rows(dim)[0])
    # strided on both sides: x in a NaN parent, out8 in a 0xFF parent
    _assert_quant(ops, F.gauss_rows(5, dim, seed=2), x_extra=8, out_extra=16)
    _assert_quant(ops, F.hand_rows(dim)[0], x_extra=24, out_extra=8)


def test_quant_fp8_grad_zero_rows_and_the_wrapper(ops):
    rc, _, _, what = _quant_call(ops, torch.zeros((0, 64), dtype=BF))
    assert rc == 0, what
    x = torch.cat([F.gauss_rows(9, 264, seed=4), F.hand_rows(264)[0]])
    c, s = ops.quant_fp8_grad(x.cuda())
    wc, ws = F.quant_grad_ref(x)
    assert c.dtype == torch.float8_e4m3fn and torch.equal(c.cpu().view(torch.uint8), wc) and _same_scales(s.cpu(), ws)
    wide = torch.full((9, 528), math.nan, dtype=BF)
    wide[:, :264] = x[:9]
    c2, s2 = ops.quant_fp8_grad(wide.cuda()[:, :264])                          # a column slice: the row stride goes to the kernel
    assert torch.equal(c2.cpu().view(torch.uint8), wc[:9]) and _same_scales(s2.cpu(), ws[:9])
    from goal_force_amd._lib import GoalForceError
    with pytest.raises(GoalForceError, match="quant_fp8_grad.x: expected dtype"):
        ops.quant_fp8_grad(x.cuda().float())
    with pytest.raises(GoalForceError, match="quant_fp8_grad.x: tensor must be on the GPU"):
        ops.quant_fp8_grad(x)
    with pytest.raises(GoalForceError, match="gf_quant_fp8_grad: dim=12 must be a multiple of 8"):
        ops.quant_fp8_grad(torch.zeros((2, 12), dtype=BF, device="cuda"))


def test_quant_fp8_grad_refusals_leave_the_outputs_untouched(ops):
    lib = _lib(ops)
    x = torch.ones((4, 64), dtype=BF, device="cuda")
    out = torch.full((4 * 64 + 16,), FILL8, dtype=torch.uint8, device="cuda")
    sc = torch.full((8,), -7.5, dtype=torch.float32, device="cuda")
    xp, op, sp, st = x.data_ptr(), out.data_ptr(), sc.data_ptr(), _st()
    for args, msg in [((None, op, sp, 4, 64, 64, 64), "null pointer"), ((xp, None, sp, 4, 64, 64, 64), "null pointer"),
                      ((xp, op, None, 4, 64, 64, 64), "null pointer"), ((xp, op, sp, -1, 64, 64, 64), "null pointer"),
                      ((xp, op, sp, 4, 0, 64, 64), "dim=0 must be a multiple of 8"), ((xp, op, sp, 4, 60, 64, 64), "dim=60 must be a multiple of 8"),
                      ((xp, op, sp, 1, 14344, 14344, 14344), "dim=14344 must be a multiple of 8 and <= 14336"),
                      ((xp, op, sp, 4, 64, 56, 64), "row strides 56 / 64 below dim=64"), ((xp, op, sp, 4, 64, 64, 56), "row strides 64 / 56 below dim=64"),
                      ((xp, op, sp, 2, 64, 68, 64), "alignment"), ((xp, op, sp, 2, 64, 64, 68), "alignment"),
                      ((xp + 2, op, sp, 2, 64, 64, 64), "alignment"), ((xp, op + 4, sp, 2, 64, 64, 64), "alignment")]:
        assert lib.gf_quant_fp8_grad(*args, st) != 0, args
        assert "gf_quant_fp8_grad: " + msg in _err(ops), (args, _err(ops))
    torch.cuda.synchronize()
    assert bool((out == FILL8).all()) and bool((sc == -7.5).all())


# ---------------------------------------------------------------------------------------------------------------------
# b. gf_cast_fp8_t, raw C ABI
def _cast_t_call(ops, w, ldw_extra=0, ldo_extra=0):
    N, K = w.shape
    ldw, ldo = K + ldw_extra, N + ldo_extra
    src = torch.full((N * ldw + 8,), NAN_BITS, dtype=torch.int16)
    src[:N * ldw].view(N, ldw)[:, :K] = w.view(torch.int16)
    dst = torch.full((GUARD + K * ldo + GUARD,), FILL8, dtype=torch.uint8)
    psrc, pdst = src.cuda(), dst.cuda()
    rc = _lib(ops).gf_cast_fp8_t(psrc.data_ptr(), ldw, pdst.data_ptr() + GUARD, ldo, N, K, _st())
    out = pdst.cpu()
    what = f"cast_fp8_t N={N} K={K} ldw={ldw} ldo={ldo}"
    assert rc == 0, f"{what}: {_err(ops)}"
    assert bool((out[:GUARD] == FILL8).all()) and bool((out[GUARD + K * ldo:] == FILL8).all()), f"{what}: a byte around out8 was written"
    body = out[GUARD:GUARD + K * ldo].view(K, ldo)
    assert bool((body[:, N:] == FILL8).all()), f"{what}: bytes [N, ldo) of a row were written"
    return body[:, :N].contiguous(), what


def _weights(N, K, seed):
    """Gaussian weights with a band of large values: codes over the whole e4m3 range, the NaN code above 464 included."""
    g = torch.Generator().manual_seed(31 * N + K + seed)
    w = torch.randn((N, K), generator=g) * torch.exp2(torch.randint(-12, 10, (N, K), generator=g).float())
    return w.to(BF)


@pytest.mark.parametrize("N", [128, 256, 640])
def test_cast_fp8_t_is_the_cast_transposed(ops, N):
    for K in (8, 64, 72, 200, 256, 520):
        w = _weights(N, K, 0)
        want_dev = ops.cast_fp8(w.cuda()).t().contiguous().cpu().view(torch.uint8)
        assert torch.equal(want_dev, F.cast_t_ref(w)), "gf_cast_fp8 against torch's cast"
        assert bool(((want_dev & 0x7F) == 0x7F).any()) or K < 64, "the data reach the NaN code"
        for kw in ({}, dict(ldw_extra=8), dict(ldo_extra=16), dict(ldw_extra=24, ldo_extra=48)):
            got, what = _cast_t_call(ops, w, **kw)
            assert torch.equal(got, want_dev), f"{what}: differs at {torch.nonzero(got != want_dev)[:4].tolist()}"
        t = ops.cast_fp8_t(w.cuda())
        assert t.dtype == torch.float8_e4m3fn and tuple(t.shape) == (K, N) and torch.equal(t.cpu().view(torch.uint8), want_dev)


def test_cast_fp8_t_on_every_bf16_value(ops):
    w = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF).reshape(256, 256)
    got, what = _cast_t_call(ops, w)
    assert torch.equal(got, ops.cast_fp8(w.cuda()).t().contiguous().cpu().view(torch.uint8)), what
    assert torch.equal(got, F.cast_t_ref(w)), what + ": torch's codes"


def test_cast_fp8_t_refusals_leave_the_output_untouched(ops):
    from goal_force_amd._lib import GoalForceError
    lib = _lib(ops)
    w = torch.ones((128, 64), dtype=BF, device="cuda")
    out = torch.full((64 * 160 + 32,), FILL8, dtype=torch.uint8, device="cuda")
    wp, op, st = w.data_ptr(), out.data_ptr(), _st()
    for args, msg in [((None, 64, op, 128, 128, 64), "null pointer"), ((wp, 64, None, 128, 128, 64), "null pointer"),
                      ((wp, 64, op, 128, 64, 64), "N=64 must be a multiple of 128"), ((wp, 64, op, 128, 0, 64), "N=0 must be a multiple of 128"),
                      ((wp, 64, op, 128, 128, 60), "K=60 a multiple of 8"), ((wp, 64, op, 128, 128, 0), "K=0 a multiple of 8"),
                      ((wp, 56, op, 128, 128, 64), "ldw=56 must be >= K"), ((wp, 68, op, 128, 128, 64), "ldw=68 must be >= K and a multiple of 8"),
                      ((wp, 64, op, 112, 128, 64), "ldo=112 >= N"), ((wp, 64, op, 136, 128, 64), "ldo=136 >= N and a multiple of 16"),
                      ((wp + 2, 64, op, 128, 128, 64), "alignment"), ((wp, 64, op + 8, 128, 128, 64), "alignment")]:
        assert lib.gf_cast_fp8_t(*args, st) != 0, args
        assert "gf_cast_fp8_t: " in _err(ops) and msg in _err(ops), (args, _err(ops))
    torch.cuda.synchronize()
    assert bool((out == FILL8).all())
    with pytest.raises(GoalForceError, match="cast_fp8_t.w: expected 2-D with contiguous rows"):
        ops.cast_fp8_t(w.t())
    with pytest.raises(GoalForceError, match="cast_fp8_t.w: expected dtype"):
        ops.cast_fp8_t(w.float())
    with pytest.raises(GoalForceError, match="gf_cast_fp8_t: N=64"):
        ops.cast_fp8_t(w[:64])


# ---------------------------------------------------------------------------------------------------------------------
# c. training.linear_dx_fp8
def _fp8_linear(w):
    from goal_force_amd import dit
    lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=False).to(BF).cuda()
    with torch.no_grad():
        lin.weight.copy_(w)
    lin.weight.requires_grad_(False)
    dit.weight_copy(lin, "fp8", True)
    return lin


@pytest.mark.parametrize("M", F.DX_M)
def test_linear_dx_fp8(ops, M):
    from goal_force_amd import dit, training
    for N, K in F.DX_WEIGHTS:
        for cls in T.LIN_CLASSES:
            dy, w = F.dx_inputs(cls, M, N, K, seed=2)
            lin = _fp8_linear(w.cuda())
            assert getattr(lin, "_gf_w8t", None) is None, "the transposed copy is made by the first backward, not by enable_fp8"
            got = training.linear_dx_fp8(dy.cuda(), lin).cpu()
            what = f"linear_dx_fp8 {cls} M={M} W {N}x{K}"
            assert got.dtype == BF and tuple(got.shape) == (M, K)
            d8, s = ops.quant_fp8_grad(dy.cuda())
            wt8 = dit.fp8_weight_t(lin)
            assert wt8 is lin._gf_w8t and torch.equal(wt8.cpu().view(torch.uint8), F.cast_t_ref(w)), what
            d8, s = d8.cpu().view(torch.uint8), s.cpu()
            if cls == "gauss":      # the exact chain on the device's own codes, through gemm_refs' two fp8 bars (test_gemm_pinned_gpu.py's way)
                ref = GR.reference(dict(a=d8, w=wt8.cpu().view(torch.uint8), bias=None, resid=None, gate=None, rs=s), GR.EPI_BIAS)
                GR.assert_pinned(got, ref, N, what)
            else:                   # every code, every product and every sum is exact: equal bits
                want = (dy.double() @ w.to(F.E4M3).double()).to(BF)
                assert torch.equal((dy.double() @ w.to(F.E4M3).double()), want.double()), what + ": the class is not exact"
                assert torch.equal(_bits(got), _bits(want)), f"{what}: {int((_bits(got) != _bits(want)).sum())} elements differ from the exact dX"


def test_linear_dx_fp8_a_nan_row_of_dy_is_a_nan_row_of_dx_and_no_other(ops):
    from goal_force_amd import training
    dy, w = F.dx_inputs("gauss", 65, 256, 512, seed=3)
    lin = _fp8_linear(w.cuda())
    clean = training.linear_dx_fp8(dy.cuda(), lin).cpu()
    bad = dy.clone()
    bad[7, 100], bad[40, 3] = math.nan, math.inf
    got = training.linear_dx_fp8(bad.cuda(), lin).cpu()
    rows = torch.isnan(got.float()).all(1)
    assert rows.nonzero().flatten().tolist() == [7, 40], "exactly the two bad rows come out NaN, whole"
    keep = ~rows
    assert torch.equal(_bits(got[keep]), _bits(clean[keep])) and not bool(torch.isnan(clean.float()).any())


# ---------------------------------------------------------------------------------------------------------------------
# d. the frozen fp8 block
CASES = {c["name"]: c for c in T.cases()}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs, fp64 dx of the straight-through fp8 block, restatement of order 0: (out, dx)) — computed once on the host."""
    import gen_inputs as gi
    case = CASES[name]
    cfg, sd, x, ctx, t_mod, dout = T.case_inputs(case, gi)
    ref = F.block_grads_ref(cfg, sd, x, ctx, t_mod, dout, case["grid"])
    c0 = F.block_chain_fp8(cfg, sd, x, ctx, t_mod, dout, case["grid"], 0, case["prescale"])
    return (cfg, sd, x, ctx, t_mod, dout), ref, c0


def _block(cfg, sd, fp8=True):
    from goal_force_amd import dit
    blk = dit.DiTBlock(False, cfg["dim"], cfg["num_heads"], cfg["ffn_dim"], cfg["eps"])
    blk.load_state_dict(sd, strict=True)
    blk = blk.to(BF).cuda()
    for p_ in blk.parameters():
        p_.requires_grad_(False)
    return dit.enable_fp8(blk) if fp8 else blk


def _rope(cfg, case):
    from goal_force_amd.dit import RopeTable, precompute_freqs_cis_3d
    return RopeTable.from_grid(precompute_freqs_cis_3d(cfg["dim"] // cfg["num_heads"]), *case["grid"], "cuda")


def _run(ops, blk, case, inputs, level, monkeypatch):
    """(out, dx) of training.block_forward + backward on a block, at a keep level."""
    from goal_force_amd import training
    cfg, sd, x, ctx, t_mod, dout = inputs
    monkeypatch.setattr(training, "KEEP_ATTENTION", True)                  # (restores the module state after the test)
    monkeypatch.setattr(training, "KEEP_WIDE", False)
    monkeypatch.setattr(training, "KEEP_AUTO", True)
    training.set_keep_level(level)
    xc = x.cuda().requires_grad_(True)
    with ops.options(attn_q_prescale=case["prescale"]):
        y = training.block_forward(blk, xc, ctx.cuda(), t_mod.cuda(), _rope(cfg, case))
        y.backward(dout.cuda())
    assert all(p_.grad is None for p_ in blk.parameters())
    return y.detach().cpu(), xc.grad.cpu()


@pytest.mark.parametrize("level", ["none", "attn", "wide"])
@pytest.mark.parametrize("name", list(CASES))
def test_frozen_fp8_block_tape_every_token_row(ops, name, level, monkeypatch):
    from goal_force_amd import training
    inputs, ref, (out0, dx0) = _case(name)
    case, (cfg, sd, x, ctx, t_mod, dout) = CASES[name], inputs
    blk = _block(cfg, sd)
    training.set_fp8_frozen(True)
    out, dx = _run(ops, blk, case, inputs, level, monkeypatch)
    with torch.no_grad(), ops.options(attn_q_prescale=case["prescale"]):
        inference = blk(x.cuda(), ctx.cuda(), t_mod.cuda(), _rope(cfg, case)).cpu()
    assert torch.equal(_bits(out), _bits(inference)), f"{name} keep={level}: the tape's forward is not the inference forward of the block"
    F.assert_rows({"dx": dx}, {"dx": dx0}, {"dx": ref}, f"fp8-frozen block {name} keep={level}")
    out2, dx2 = _run(ops, blk, case, inputs, level, monkeypatch)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(dx), _bits(dx2)), f"{name} keep={level}: two calls, two results"


def test_frozen_fp8_block_follows_an_in_place_update_of_a_master_weight(ops, monkeypatch):
    from goal_force_amd import dit, training
    inputs, _, _ = _case(T.BASE_CASE)
    case, (cfg, sd, x, ctx, t_mod, dout) = CASES[T.BASE_CASE], inputs
    blk = _block(cfg, sd)
    training.set_fp8_frozen(True)
    _run(ops, blk, case, inputs, "attn", monkeypatch)
    lin = blk.ffn[0]
    old8, old8t = lin._gf_w8.clone(), lin._gf_w8t.clone()
    with torch.no_grad():
        lin.weight.mul_(0.75)
        blk.self_attn.k.weight.add_(0.01)
    out, dx = _run(ops, blk, case, inputs, "attn", monkeypatch)
    assert not torch.equal(lin._gf_w8.view(torch.uint8), old8.view(torch.uint8)) and not torch.equal(lin._gf_w8t.view(torch.uint8), old8t.view(torch.uint8))
    assert torch.equal(lin._gf_w8t.view(torch.uint8), ops.cast_fp8(lin.weight.detach()).t().contiguous().view(torch.uint8))
    sd2 = {k: v.detach().cpu() for k, v in blk.state_dict().items()}
    fresh_out, fresh_dx = _run(ops, _block(cfg, sd2), case, inputs, "attn", monkeypatch)
    assert torch.equal(_bits(out), _bits(fresh_out)) and torch.equal(_bits(dx), _bits(fresh_dx)), "the gradient is not the fresh model's"
    dit.enable_fp8(blk, False)
    assert all(getattr(m, "_gf_w8t", None) is None and getattr(m, "_gf_w8", None) is None for m in blk.modules())


def test_frozen_fp8_block_refusals(ops, monkeypatch):
    from goal_force_amd import training
    from goal_force_amd._lib import GoalForceError
    inputs, _, _ = _case(T.BASE_CASE)
    case, (cfg, sd, x, ctx, t_mod, dout) = CASES[T.BASE_CASE], inputs
    blk = _block(cfg, sd)
    with pytest.raises(GoalForceError) as e:                                # the switch off: word for word what it was
        training.block_forward(blk, x.cuda().requires_grad_(True), ctx.cuda(), t_mod.cuda(), _rope(cfg, case))
    assert str(e.value) == "training through an enable_fp8 block is refused: call enable_fp8(module, False) first"
    training.set_fp8_frozen(True)
    blk.norm3.weight.requires_grad_(True)
    with pytest.raises(GoalForceError, match=r"frozen blocks only.*the trainable parameter norm3\.weight"):
        training.block_forward(blk, x.cuda().requires_grad_(True), ctx.cuda(), t_mod.cuda(), _rope(cfg, case))
    blk.norm3.weight.requires_grad_(False)
    _run(ops, blk, case, inputs, "none", monkeypatch)                       # frozen again: accepted


# ---------------------------------------------------------------------------------------------------------------------
# e. the step: an fp8-frozen expert under a two-layer bf16 ControlNet
@functools.lru_cache(maxsize=None)
def _model_case(zero):
    import gen_inputs as gi
    cfg, inp = gi.TINY, gi.train_inputs()
    dit_sd, cn_sd = gi.dit_sd(cfg, seed=41), gi.controlnet_sd(cfg, 2, seed=42, zero_convs_zero=zero)
    args = (cfg, dit_sd, cn_sd, 2, inp, gi.TRAIN_TIMESTEP_ID)
    return args, F.model_grads_ref(*args), F.model_chain_fp8(*args, order=0)


def _pipe(cfg, dit_sd, cn_sd, n_cn):
    from goal_force_amd.controlnet import ControlNet
    from goal_force_amd.dit import WanModel
    from goal_force_amd.pipeline import WanVideoPipeline
    dit = WanModel(has_image_input=False, require_clip_embedding=False, **cfg)
    dit.load_state_dict(dit_sd, strict=True)
    cn = ControlNet(n_cn, dim=cfg["dim"], num_heads=cfg["num_heads"], ffn_dim=cfg["ffn_dim"])
    cn.load_state_dict(cn_sd, strict=True)
    pipe = WanVideoPipeline.from_modules(dit.to(BF).cuda(), None, cn.to(BF).cuda(), None, device="cuda")
    pipe.scheduler.set_timesteps(1000, training=True)
    pipe.freeze_except(["controlnet"])
    return pipe


def _loss(pipe, dev, tid):
    return pipe.training_loss(input_latents=dev["input_latents"], noise=dev["noise"], context=dev["context"], y=dev["y"],
                              control_signal_video_latents=dev["control"], timestep_id=tid)


@pytest.mark.parametrize("zero", T.MODEL_CASES)
def test_step_over_an_fp8_frozen_expert(ops, zero):
    from goal_force_amd import dit as D
    from goal_force_amd import training
    (cfg, dit_sd, cn_sd, n_cn, inp, tid), (loss_ref, g_ref, pred_ref), (l0, c0, pred0) = _model_case(zero)
    pipe = _pipe(cfg, dit_sd, cn_sd, n_cn)
    D.enable_fp8(pipe.dit)
    training.set_fp8_frozen(True)
    dev = {k: v.cuda() for k, v in inp.items()}
    masters = {k: v.detach().clone() for k, v in pipe.dit.state_dict().items()}
    loss = _loss(pipe, dev, tid)
    loss.backward()
    named = dict(pipe.controlnet.named_parameters())
    assert sorted(named) == sorted(g_ref) and all(p_.grad is None for p_ in pipe.dit.parameters()), "only ControlNet parameters carry gradients"
    got = {n: named[n].grad.cpu() for n in g_ref}
    lv = float(loss.detach())
    bar = F.loss_bar(loss_ref, pred_ref, pred0, inp)
    print(f"LOSS device {lv:.7f} fp64 {loss_ref:.7f} restatement {l0:.7f}: {abs(lv - loss_ref):.2e} from fp64 (restatement {abs(l0 - loss_ref):.2e}, bar {bar:.2e})")
    if zero:
        for n, t in got.items():
            if "zero_convs" not in n:
                assert not bool(t.any()), f"{n}: behind zero convs every ControlNet gradient is exactly zero"
    F.assert_rows(got, c0, g_ref, f"fp8-frozen step zero_convs_zero={zero}", model=True)
    assert abs(lv - loss_ref) <= bar, f"the loss is {abs(lv - loss_ref):.3e} from fp64, bar {bar:.3e}"
    opt = training.AdamW(list(pipe.controlnet.parameters()), lr=1e-3)
    opt.step()
    after = pipe.dit.state_dict()
    assert all(torch.equal(_bits(masters[k]), _bits(after[k])) for k in masters), "an expert master moved under the optimiser"
    assert all(D.precision(m) == "fp8" for b in pipe.dit.blocks for m in b.modules() if isinstance(m, torch.nn.Linear))


def test_train_script_path_with_enable_fp8_training(ops, tmp_path):
    """scripts/train.py's own steps for `--enable_fp8_training` — parser, check_args, the freeze, enable_fp8_training — on the TINY
    pipeline, then two steps of launch_training_task through its forward= seam."""
    import datetime
    import types
    from goal_force_amd import dit as D
    from goal_force_amd import training
    spec = importlib.util.spec_from_file_location("gf_train_script_fp8_gpu", os.path.join(ROOT, "scripts", "train.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    (cfg, dit_sd, cn_sd, n_cn, inp, tid), _, _ = _model_case(False)
    cli = script.parser().parse_args(["--dataset_base_path", "x", "--control_signal_type", "canny_edge", "--trainable_models", "controlnet",
                                      "--enable_fp8_training"])
    script.check_args(cli)
    pipe = _pipe(cfg, dit_sd, cn_sd, n_cn)
    pipe.freeze_except(cli.trainable_models.split(","))
    assert script.enable_fp8_training(pipe, cli) == 1 and training.FP8_FROZEN is True
    assert all(D.precision(b.self_attn.q) == "fp8" for b in pipe.dit.blocks)
    assert all(D.precision(b.self_attn.q) == "bf16" for b in pipe.controlnet.controlnet_dit.blocks)
    dev = {k: v.cuda() for k, v in inp.items()}
    args = types.SimpleNamespace(learning_rate=1e-3, weight_decay=1e-2, dataset_num_workers=0, save_steps=None, num_epochs=1,
                                 gradient_accumulation_steps=1, output_path=str(tmp_path), remove_prefix_in_ckpt="pipe.dit.",
                                 control_signal_type="canny_edge", num_frames=5, max_grad_norm=1.0, controlnet_checkpoint=None)
    control = torch.zeros(5, 480, 832, 3, dtype=torch.uint8)
    items = [dict(video=[], control_video=control, file_id=str(i)) for i in range(2)]
    before = {k: v.detach().clone() for k, v in pipe.controlnet.state_dict().items()}
    seen = []

    def forward(p_, data):
        seen.append(_loss(p_, dev, tid))
        return seen[-1]

    logger = training.launch_training_task(items, pipe, args=args, forward=forward, shuffle=False, now=datetime.datetime(2026, 1, 2, 3, 4, 5))
    assert logger.num_steps == 2 and all(math.isfinite(float(v.detach())) for v in seen)
    after = pipe.controlnet.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before), "the ControlNet did not move"
    # the backward ran on the transposed fp8 copies — of the blocks behind the first injection: block 0's input carries no gradient, its
    # backward never runs, and the lazy copy is never made
    assert all(getattr(b.ffn[0], "_gf_w8t", None) is not None for b in pipe.dit.blocks[1:]) and getattr(pipe.dit.blocks[0].ffn[0], "_gf_w8t", None) is None
