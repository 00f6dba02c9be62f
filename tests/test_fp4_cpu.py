"""MXFP4 without a GPU: the quantiser's recipe (include/goalforce.h) on hand-made blocks, the declarations of the two entry points,
enable_fp4's bookkeeping on a CPU-constructed block, and the sensitivity of the GPU test's two bars: on every random input
tests/test_fp4_gpu.py draws, the fp32 restatement (fp4_refs.gemm_f32) stays inside both bars of gemm_refs.judge in both block orders and
through the model of the instruction, and each injected fault lands outside one of them.
"""
import os
import re

import pytest
import torch

import fp4_refs as F
import gemm_refs as R

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _block(values, fill=0.0):
    """One 32-element block [1, 32] bf16: `values` first, `fill` after."""
    v = list(values) + [fill] * (32 - len(values))
    return torch.tensor([v], dtype=torch.float64).to(BF)


def _q(x):
    p, s = F.quantize(x)
    return F.unpack(p)[0].tolist(), int(s[0, 0])


# ---------------------------------------------------------------------------------------------------------------------
# the quantiser
def test_every_e2m1_value_and_the_packing():
    grid = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    x = _block(grid + [-v for v in grid])
    codes, scale = _q(x)
    assert scale == 127 and codes[:8] == list(range(8)) and codes[8:16] == [8 + c for c in range(8)]     # -0.0 keeps its sign bit
    p, _ = F.quantize(x)
    assert p[0, 0] == (1 << 4) | 0 and p[0, 1] == (3 << 4) | 2 and p[0, 3] == (7 << 4) | 6       # element 2i low nibble, 2i + 1 high
    assert torch.equal(F.decode(*F.quantize(x)), x.double())


def test_every_tie_goes_to_the_even_mantissa_code_and_7_saturates():
    # amax = 6 keeps the scale at 1: the ties of the grid 0, .5, 1, 1.5, 2, 3, 4, 6
    ties = {0.25: 0.0, 0.75: 1.0, 1.25: 1.0, 1.75: 2.0, 2.5: 2.0, 3.5: 4.0, 5.0: 4.0}
    x = _block([6.0] + list(ties) + [-t for t in ties])
    got = F.decode(*F.quantize(x))[0]
    assert got[0] == 6.0
    assert got[1:8].tolist() == list(ties.values()) and got[8:15].tolist() == [-v for v in ties.values()]
    assert torch.signbit(got[8]) and got[8] == 0.0                                                # -0.25 -> -0
    # just off the ties
    x = _block([6.0, 0.251, 0.249, 5.03, 4.97, 2.51, 2.49])
    assert F.decode(*F.quantize(x))[0, :7].tolist() == [6.0, 0.5, 0.0, 6.0, 4.0, 3.0, 2.0]
    # 7 (amax 7: floor(log2) = 2, scale 1) saturates at 6; so does 7.96875, the largest bf16 below 8
    assert _q(_block([7.0, -7.0, 6.5, 7.96875])) == ([7, 15, 7, 7] + [0] * 28, 127)


def test_scale_at_and_one_bf16_step_around_a_power_of_two():
    for p in (-20, 0, 1, 9):
        two = 2.0 ** p
        below, above = two * (1 - 2.0 ** -8), two * (1 + 2.0 ** -7)          # the neighbouring bf16 values
        assert _q(_block([two]))[1] == 127 + p - 2 and _q(_block([above]))[1] == 127 + p - 2
        assert _q(_block([below]))[1] == 127 + p - 3
        # at amax = 2^p the element is 4; one step below, 7.97 at the smaller scale saturates to 6
        assert _q(_block([two]))[0][0] == 6 and _q(_block([below]))[0][0] == 7


def test_zero_block_and_signs_of_zero():
    assert _q(torch.zeros((1, 32), dtype=BF)) == ([0] * 32, 127)
    assert _q(-torch.zeros((1, 32), dtype=BF)) == ([0] * 32, 127)            # amax = 0: all elements +0


def test_subnormal_block_and_the_clamps_of_e8m0():
    tiny = 2.0 ** -133                                                       # bf16's smallest subnormal
    x = _block([tiny * 127, tiny, -tiny * 64, tiny * 16, tiny * 8])
    assert float(x[0, 1]) == tiny and float(x[0, 0]) == tiny * 127            # not flushed
    codes, scale = _q(x)
    # floor(log2(127 2^-133)) - 2 + 127 = -129 + 127 < 0: clamped to code 0 = 2^-127; 127 2^-133 / 2^-127 = 1.98 -> 2, 2^-6 -> 0, -1, .25 -> 0, .125 -> 0
    assert scale == 0 and codes[:5] == [4, 0, 8 | 2, 0, 0]
    # the smallest normal exponents clamp too: exponent fields 1, 2 -> code 0; field 3 -> code 1
    assert _q(_block([2.0 ** -126]))[1] == 0 and _q(_block([2.0 ** -125]))[1] == 0 and _q(_block([2.0 ** -124]))[1] == 1
    assert _q(_block([2.0 ** -125]))[0][0] == 6                               # 2^-125 / 2^-127 = 4
    # the upper end: bf16's largest finite value has floor(log2) = 127 -> code 252; 253 and 254 cannot be reached from bf16 and the
    # clamp at 254 is never active; 255 is the NaN code only
    big = torch.tensor([[0x7F7F] + [0] * 31], dtype=torch.int32).to(torch.int16).view(BF)
    codes, scale = _q(big)
    assert scale == 252 and codes[0] == 7                                     # 1.992 2^127 / 2^125 = 7.97 -> 6


def test_nan_and_inf_give_the_nan_code_and_zero_elements():
    for bad in (float("nan"), float("inf"), float("-inf")):
        x = torch.cat([_block([1.0, bad, -3.0]), _block([1.0, 2.0])], 1)
        p, s = F.quantize(x)
        assert s.tolist() == [[255, 126]] and F.unpack(p)[0, :32].tolist() == [0] * 32 and F.unpack(p)[0, 32:34].tolist() == [4, 6]
        assert bool(torch.isnan(F.decode(p, s)[0, :32]).all())


def test_quantising_the_dequantised_values_is_idempotent():
    g = torch.Generator().manual_seed(5)
    x = torch.cat([(torch.randn((64, 256), generator=g) * s).to(BF) for s in (1e-3, 1.0, 1e3)])
    x[3, 32:64] = 0
    p, s = F.quantize(x)
    back = F.decode(p, s)
    assert torch.equal(back.to(BF).double(), back)                            # every MXFP4 value is a bf16 value
    p2, s2 = F.quantize(back.to(BF))
    # a block whose maximum rounded UP to the next binade (7 -> ... no: saturation keeps 6) keeps its scale: 6 s has the exponent of amax
    assert torch.equal(s2, s) and torch.equal(F.decode(p2, s2), back)
    live = F.unpack(p) & 7
    assert torch.equal(F.unpack(p2) & 7, live) and torch.equal((F.unpack(p2) >> 3)[live > 0], (F.unpack(p) >> 3)[live > 0])


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_header_declares_the_entry_points_and_the_bindings_have_them():
    from goal_force_amd import _lib
    text = " ".join(open(os.path.join(ROOT, "include", "goalforce.h"), encoding="utf-8").read().split())
    quant = ("GF_API int gf_quant_mxfp4(const void* x, int64_t x_stride, void* out4, int64_t out_stride, void* scales, int64_t scale_stride, "
             "int64_t rows, int64_t dim, void* stream);")
    gemm = ("GF_API int gf_gemm_mxfp4(const void* A4, int64_t lda, const void* a_scale, int64_t a_scale_stride, const void* W4, int64_t ldw, "
            "const void* w_scale, int64_t w_scale_stride, const void* bias, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K, int epilogue, "
            "const void* resid, int64_t ldr, const void* gate, void* stream);")
    assert quant in text and gemm in text
    import ctypes
    p, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert _lib.BINDINGS["gf_quant_mxfp4"] == (i, [p, i64, p, i64, p, i64, i64, i64, p])
    assert _lib.BINDINGS["gf_gemm_mxfp4"] == (i, [p, i64, p, i64, p, i64, p, i64, p, p, i64, i64, i64, i64, i, p, i64, p, p])
    assert _lib.ABI_VERSION == 20 and re.search(r"^#define GF_ABI_VERSION 20\s*$", open(_lib.HEADER_PATH).read(), flags=re.M)


# ---------------------------------------------------------------------------------------------------------------------
# enable_fp4's bookkeeping (the two quantisers replaced by CPU stand-ins: the attributes are what is looked at)
@pytest.fixture
def dit(monkeypatch):
    from goal_force_amd import dit as _dit, ops
    monkeypatch.setattr(ops, "quant_mxfp4", lambda w: F.quantize(w))
    monkeypatch.setattr(ops, "cast_fp8", lambda w: w.to(torch.float8_e4m3fn))
    return _dit


def _carriers(blk, attr):
    return sorted(name for name, m in blk.named_modules() if getattr(m, attr, None) is not None)


def test_enable_fp4_bookkeeping_on_a_cpu_block(dit):
    from goal_force_amd._lib import GoalForceError
    blk = dit.DiTBlock(False, 256, 2, 512).to(BF)
    every = sorted(name for name, m in blk.named_modules() if isinstance(m, torch.nn.Linear))
    ffn, o = ["ffn.0", "ffn.2"], ["cross_attn.o", "self_attn.o"]
    assert _carriers(blk, "_gf_w4") == []
    assert dit.enable_fp4(blk) is blk and _carriers(blk, "_gf_w4") == sorted(ffn + o)
    p, s = blk.ffn[0]._gf_w4
    assert p.dtype == s.dtype == torch.uint8 and tuple(p.shape) == (512, 128) and tuple(s.shape) == (512, 8)
    assert torch.equal(F.decode(p, s), F.fake_quant(blk.ffn[0].weight.detach()))
    dit.enable_fp4(blk, False, layers=("o",))
    assert _carriers(blk, "_gf_w4") == ffn
    dit.enable_fp4(blk, False)
    assert _carriers(blk, "_gf_w4") == []
    dit.enable_fp4(blk, layers="ffn")
    assert _carriers(blk, "_gf_w4") == ffn
    # on top of fp8: every Linear keeps its fp8 copy, the fp4 copy wins where both exist, and False leaves the fp8 copies
    dit.enable_fp8(blk)
    assert _carriers(blk, "_gf_w8") == every and _carriers(blk, "_gf_w4") == ffn
    assert dit.fp4_weight(blk.ffn[0]) is not None and dit.fp4_weight(blk.self_attn.o) is None and dit.fp8_weight(blk.self_attn.o) is not None
    dit.enable_fp4(blk, False)
    assert _carriers(blk, "_gf_w4") == [] and _carriers(blk, "_gf_w8") == every
    dit.enable_fp8(blk, False)
    # the copy follows the bf16 master (param_key)
    dit.enable_fp4(blk, layers=("o",))
    before = blk.self_attn.o._gf_w4
    assert dit.fp4_weight(blk.self_attn.o) is before
    with torch.no_grad():
        blk.self_attn.o.weight.mul_(2.0)
    after = dit.fp4_weight(blk.self_attn.o)
    assert after is not before and torch.equal(after[0], before[0]) and torch.equal(after[1], before[1] + 1)     # x 2: the scales move
    # refusals
    for bad in (("q",), ("ffn", "v"), "k"):
        with pytest.raises(GoalForceError, match="unknown layer name"):
            dit.enable_fp4(blk, layers=bad)
    with pytest.raises(GoalForceError, match="training through an enable_fp4 block is refused: call enable_fp4\\(module, False\\) first"):
        dit.refuse_training(blk)
    dit.enable_fp4(blk, False)
    dit.refuse_training(blk)
    with pytest.raises(GoalForceError, match="multiple of 256"):
        dit.enable_fp4(dit.DiTBlock(False, 128, 1, 512).to(BF))


def test_enable_fp4_reaches_the_blocks_of_a_container(dit):
    holder = torch.nn.Module()
    holder.blocks = torch.nn.ModuleList([dit.DiTBlock(False, 256, 2, 512).to(BF) for _ in range(2)])
    dit.enable_fp4(holder, layers=("ffn",))
    assert all(_carriers(b, "_gf_w4") == ["ffn.0", "ffn.2"] for b in holder.blocks)


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity of the GPU test's bars (gemm_refs.judge) on the GPU test's own random inputs
_REFS = {}


def _gauss(M, N, K):
    if (M, N, K) not in _REFS:
        _REFS[(M, N, K)] = F.gauss_inputs(M, N, K)
    return _REFS[(M, N, K)]


@pytest.mark.parametrize("M,N,K", F.SHAPES + F.EXTRA_SHAPES)
def test_restatement_stays_inside_both_bars_on_every_gauss_input(M, N, K):
    d = _gauss(M, N, K)
    for epi in R.EPIS:
        r = F.reference(d, epi)
        assert bool((r.T >= 0).all()) and float((r.T / r.S.clamp_min(1e-30)).max()) < 2.0 ** -18, "on quantiser operands T is a few fp32 ulps of S"
        for how in F.ORDERS + ("mfma",):
            j = R.judge(F.gemm_f32(d, epi, how), r, K)
            assert R.passes(j) == (True, True), f"{M} x {N} x {K} {R.EPI_NAMES[epi]} {how}: {R.describe(j)}"


FAULT_SHAPES = [(513, 520, 1280), (257, 264, 1280), (129, 264, 512)]


@pytest.mark.parametrize("fault", F.FAULTS)
def test_each_fault_lands_outside_a_bar(fault):
    for (M, N, K) in FAULT_SHAPES:
        if fault == "row_2pct" and M != 513:
            continue                                           # one row 2 % off at the largest M
        d = _gauss(M, N, K)
        for epi in (R.EPI_BIAS, R.EPI_GATE_RESID):
            j = R.judge(F.gemm_f32(d, epi, "kloop", fault=fault), F.reference(d, epi), K)
            assert R.passes(j) != (True, True), f"{fault} at {M} x {N} x {K} {R.EPI_NAMES[epi]} passes both bars: {R.describe(j)}"


def test_integer_and_layout_classes_are_what_they_claim():
    for (M, N, K) in [(257, 264, 768), (513, 520, 256), (17, 56, 1280)]:
        d = F.integer_inputs(M, N, K)
        acc, _ = F.product(*F.operands(d))
        for how in F.ORDERS + ("mfma",):
            for epi in (R.EPI_BIAS, R.EPI_GATE_RESID, R.EPI_RESID, R.EPI_MUL):
                assert torch.equal(F.bits(F.gemm_f32(d, epi, how)), F.bits(F.reference(d, epi).out)), (M, N, K, how, epi)
    d = F.selector_inputs(513, 264, 512)
    assert set(d["k"].tolist()) == set(range(512))
    acc, S = F.product(*F.operands(d))
    assert torch.equal(acc.abs(), S) and torch.equal(acc.to(BF).double(), acc)
    for fault in ("swapped_nibbles", "scales_shifted_one_block", "scale_from_next_row"):
        a4, sa, w4, sw = F._faulty_operands(d, fault)
        assert not torch.equal(F.product(a4, sa, w4, sw)[0], acc), fault
