"""tests/gemm_refs.py on the CPU: the chain is torch's own bf16 arithmetic where torch rounds at the same points, the vt32 layout is the
permutation written out key by key, the fp32 restatement (both K orders) is inside both bars on every random input of
tests/test_gemm_pinned_gpu.py, and each injected fault is outside at least one — two of them inside the whole-tensor bars the suite
had before.  No GPU; every comparison prints what it measured (`pytest -s`)."""
import math
from fractions import Fraction

import pytest
import torch
import torch.nn.functional as F

import gemm_refs as R

BF = torch.bfloat16


def _ref(d, epi):
    return R.reference(d, epi)


def _restate(d, epi, order=0, fault=None, ktile=None):
    ktile = ktile or (128 if d["a"].dtype == torch.uint8 else 64)
    return R.gemm_f32(d["a"], d["w"], d["bias"], epi, d["resid"], d["gate"], d["rs"], ktile, order, fault,
                      mfma=R.mfma_of(d)[0] if d["a"].dtype == torch.uint8 and "k" not in d else False)


def test_activation_slopes_stay_below_L():
    x = torch.arange(-16 * 1024, 16 * 1024 + 1, dtype=torch.float64) / 1024
    for kind, L, peak in (("silu", R.L_SILU, 1.0998), ("gelu_tanh", R.L_GELU, 1.1290)):
        with torch.enable_grad():
            xg = x.clone().requires_grad_(True)
            (g,) = torch.autograd.grad(R.act_ref(xg, kind).sum(), xg)
        print(f"largest slope of {kind}: {float(g.abs().max()):.5f} at x = {float(x[g.abs().argmax()]):.4f} (L = {L})")
        assert abs(float(g.abs().max()) - peak) < 2e-4 and float(g.abs().max()) <= L


def test_cap_is_the_binomial_tail():
    p = Fraction(1, 1024)
    for n in (8, 264, 776, 2305):
        c = R.cap(n)
        tail = lambda k: 1 - sum(math.comb(n, i) * p ** i * (1 - p) ** (n - i) for i in range(k + 1))   # noqa: E731  (exact)
        print(f"cap({n}) = {c}: P[> cap] = {float(tail(c)):.2e}, P[> cap - 1] = {float(tail(c - 1)):.2e}")
        assert tail(c) < Fraction(1, 10 ** 9) <= tail(c - 1)
    assert R.cap(8) == 3 and R.cap(264) >= 6


def test_chain_is_torch_bf16_arithmetic_on_the_selector_class():
    """Every fp32 operation of the epilogue is exact before its rounding on this class, so fp64, fp32 and torch agree bit for bit; the
    activations: torch's fp32 formula equals bf16(fp64 function) except within its own error of a rounding boundary."""
    for fp8 in (False, True):
        d = R.selector_inputs(257, 264, 256 if fp8 else 192, fp8=fp8)
        acc = R.selector_acc(d)
        assert torch.equal(acc, R.product(d["a"], d["w"])[0]), "the one-hot product is w[n, k(m)]"
        if fp8:
            acc = acc * d["rs"].double()[:, None]
        y = (acc.to(BF) + d["bias"]) if not fp8 else (acc + d["bias"].double()).to(BF)
        assert torch.equal((acc + d["bias"].double()).float().double(), acc + d["bias"].double()), "w + bias is exact in fp32"
        want = {R.EPI_BIAS: y, R.EPI_GATE_RESID: d["resid"] + d["gate"] * y, R.EPI_RESID: d["resid"] + y, R.EPI_MUL: y * d["resid"],
                R.EPI_GELU: F.gelu(y, approximate="tanh"), R.EPI_SILU: F.silu(y)}
        for epi in R.EPIS:
            out = _ref(d, epi).out
            if epi in (R.EPI_GELU, R.EPI_SILU):
                # torch's GELU is 0.5 x (1 + tanh u) in fp32, which cancels for negative x: compared where it does not (x > -0.5)
                keep = (y.double() > -0.5) if epi == R.EPI_GELU else torch.ones_like(y, dtype=torch.bool)
                steps = torch.where(keep, R.bf16_steps(out.to(BF), want[epi]), 0)
                off = steps != 0
                f = R.act_ref(y, "gelu_tanh" if epi == R.EPI_GELU else "silu")
                mid = (out + want[epi].double()) / 2                        # the boundary between the two candidates
                close = ((f - mid).abs() <= 2.0 ** -19 * f.abs())[off]
                print(f"selector fp8={fp8} {R.EPI_NAMES[epi]}: torch differs from bf16(fp64) on {int(off.sum())}/{off.numel()}, all at a boundary: {bool(close.all())}")
                assert int(steps.max()) <= 1 and bool(close.all()) and float(off.double().mean()) <= R.SHARE_CAP
            else:
                assert torch.equal(R.bits(out), R.bits(want[epi])), f"{R.EPI_NAMES[epi]} fp8={fp8}: the chain is not torch's bf16 arithmetic"
                got = _restate(d, epi, order=2)
                assert torch.equal(R.bits(got), R.bits(out)), "the fp32 restatement is exact on the selector class"


def test_integer_class_is_exact_in_every_order():
    for fp8, (M, N, K) in ((False, (257, 264, 320)), (True, (257, 264, 640)), (False, (130, 264, 1024))):
        d = R.integer_inputs(M, N, K, fp8=fp8)
        for epi in (R.EPI_BIAS, R.EPI_GATE_RESID, R.EPI_RESID, R.EPI_MUL):      # the activations are a function of the exact y: gf_act's bits
            out = _ref(d, epi).out
            for order in (0, 2, 3):
                assert torch.equal(R.bits(_restate(d, epi, order)), R.bits(out)), (fp8, epi, order)


def test_vt32_layout_is_the_permutation_written_out():
    for kv in R.VT_KV:
        y = torch.arange(kv * 3, dtype=torch.float64).reshape(kv, 3) + 1
        kvp = -(-kv // 64) * 64
        want = torch.zeros((3, kvp), dtype=torch.float64)
        for s in range(kv):
            G, r = divmod(s, 32)
            g, i = divmod(r % 16, 4)
            want[:, 32 * G + 8 * g + i + (4 if r >= 16 else 0)] = y[s]
        assert torch.equal(R.vt32_layout(y, kv), want), kv
    assert sorted(R.vt_positions(128).tolist()) == list(range(128))


def _gauss_cases():
    out = [("ph", c, False) for c in R.PH_CASES] + [("a4", c, False) for c in R.A4_CASES + [R.A4_BIG]]
    out += [("a4", R.STAGGER_SHAPE + (k,), False) for k in R.BF16_K]
    out += [("f8", c, True) for c in R.F8_CASES] + [("a4f8", c, True) for c in R.A4F8_CASES + [R.A4F8_BIG]]
    out += [("a4f8", R.STAGGER_SHAPE + (k,), True) for k in R.FP8_K]
    return out


WORST = {}


@pytest.mark.parametrize("form,shape,fp8", _gauss_cases())
def test_restatement_passes_on_every_random_input_of_the_gpu_test(form, shape, fp8):
    """All six epilogues in both K orders (every column tile from K tile 0; rotated by 2 per column tile)."""
    M, N, K = shape
    d = R.gauss_inputs(M, N, K, fp8=fp8)
    for epi in R.EPIS:
        ch = _ref(d, epi)
        for order in (0, 2):
            j = R.assert_pinned(_restate(d, epi, order), ch, K, f"f32 {form} {shape} {R.EPI_NAMES[epi]} order {order}")
            w = WORST.setdefault(form, dict(share=0.0, worst=0.0, row=0.0, col=0.0))
            w.update(share=max(w["share"], j["share"]), worst=max(w["worst"], j["worst"]), row=max(w["row"], j["row_worst"] / j["row_cap"]),
                     col=max(w["col"], j["col_worst"] / j["col_cap"]))
            assert j["share"] <= R.SHARE_CAP / 4, "the random class stays where the restatement is under a quarter of the share cap"
            assert j["row_worst"] <= max(1, j["row_cap"] // 2) and j["col_worst"] <= max(1, j["col_cap"] // 2), "the random class must stay well inside the caps"
    print("restatement so far:", WORST)


def test_restatement_passes_on_the_vt32_and_batched_inputs():
    for kv, N, K in R.VT_CASES + R.VT_CASES_FP8:
        fp8 = (kv, N, K) in R.VT_CASES_FP8 and K in (128, 384)
        d = R.gauss_inputs(kv, N, K, fp8=fp8)
        got = R.vt32_layout(_restate(d, R.EPI_BIAS, order=2).double(), kv)
        R.assert_pinned(got, R.ref_map(_ref(d, R.EPI_BIAS), lambda t: R.vt32_layout(t, kv)), K, f"f32 vt32 kv={kv} N={N} K={K} fp8={fp8}")
    for B, M, N, K in R.BATCHED_CASES:
        a, w = R.batched_inputs("gauss", B, M, N, K)
        got = torch.cat([R.gemm_f32(a[b], w[b], None, R.EPI_BIAS, None, None) for b in range(B)])
        j = R.assert_pinned(got, R.batched_reference(a, w), K, f"f32 batched B={B} M={M} N={N} K={K}")
        assert j["share"] <= R.SHARE_CAP / 4


# (fault, epilogue, shape, fp8): the shape at which the fault must be outside a bar
FAULT_CASES = [("row_2pct", R.EPI_BIAS, (2305, 264, 64), False), ("bias_piece_shift", R.EPI_BIAS, (257, 264, 64), False),
               ("drop_last_ktile", R.EPI_BIAS, (129, 520, 320), False), ("no_first_rounding", R.EPI_GELU, (257, 264, 192), False),
               ("no_first_rounding", R.EPI_GATE_RESID, (257, 264, 192), False), ("gate_after_resid", R.EPI_GATE_RESID, (257, 264, 64), False),
               ("row_scale_prev", R.EPI_BIAS, (257, 264, 128), True)]


@pytest.mark.parametrize("fault,epi,shape,fp8", FAULT_CASES)
def test_each_fault_is_outside_a_bar(fault, epi, shape, fp8):
    M, N, K = shape
    d = R.gauss_inputs(M, N, K, fp8=fp8)
    ch = _ref(d, epi)
    right = R.judge(_restate(d, epi, 2), ch, K)
    assert all(R.passes(right)), R.describe(right)
    got = _restate(d, epi, 2, fault)
    j = R.judge(got, ch, K)
    a, b = R.passes(j)
    ok_old, e, frac = R.old_bars(got, ch.out.to(BF))
    print(f"FAULT {fault} {R.EPI_NAMES[epi]} {shape}: (a) {'passes' if a else 'FAILS'}, (b) {'passes' if b else 'FAILS'}: {R.describe(j)}; "
          f"old bars rel-L2 {e:.2e} (< 2e-3), > 2 ulp share {frac:.2e} (< 5e-3): {'pass' if ok_old else 'fail'}")
    assert not (a and b), f"{fault} passes both bars"
    if fault in ("row_2pct", "bias_piece_shift"):
        assert ok_old, f"{fault} was expected inside the old whole-tensor bars (rel-L2 {e:.2e}, share {frac:.2e})"
    if fault == "row_2pct":
        assert j["share"] <= R.SHARE_CAP and j["row_worst"] > j["row_cap"], "one row in 2305 is what the per-row cap is for"
    if fault == "no_first_rounding":
        print(f"  share of differing elements with the first rounding dropped: {j['share']:.3f}")
        assert j["share"] > 0.05


def test_vt32_faults_are_outside():
    kv, N, K = 300, 512, 64
    d = R.gauss_inputs(kv, N, K)
    lay = lambda t, **kw: R.vt32_layout(t, kv, **kw)                        # noqa: E731
    ref = R.ref_map(_ref(d, R.EPI_BIAS), lay)
    got = _restate(d, R.EPI_BIAS).double()
    assert all(R.passes(R.judge(lay(got), ref, K)))
    for fault in R.VT32_FAULTS:
        bad = lay(got, fault=fault, bias=d["bias"].double())
        j = R.judge(bad, ref, K)
        print(f"FAULT vt32 {fault}: {R.describe(j)}")
        assert not all(R.passes(j))
        if fault == "pad_holds_bias":
            assert not bool((bad[:, R.vt_positions(320)[kv:]] == 0).all()), "the GPU test asks the pad columns for exact zeros"
