"""The checker of the forward-kernel tests, checked on the CPU (no GPU needed).

tests/test_forward_kernels_gpu.py holds gf_rowops.hip and gf_elementwise.hip against the exact chains of tests/forward_refs.py through
two bars: (a) differing bf16 bits on at most 2^-10 of the elements, (b) every element within 2^-7 m + 2^-16 s.  This file is the evidence
that those tests mean something:
 * the fp32 restatement of every chain passes (a) and (b) on every input the GPU test uses (the case lists are shared), so a right
   kernel passes — each case prints its differing share and its worst share of the allowance (`pytest -s`, lines `PIN`);
 * each of forward_refs.FAULTS, switched on in a restatement, fails (a) or (b) — lines `FAULT` say which;
 * the exact chains equal oracle/wan_oracle.py's layer_norm / modulate / rms_norm / rope_apply (fp32 torch, what the goldens pin) to
   the same two bars, so the new helper is tied to the oracle;
 * x - mean formed with a rounded 1 / dim leaves a constant row non-zero at 5120 and 1536 and fails both bars: why the wave-per-row
   LayerNorm kernels divide.
"""
import pytest
import torch

import forward_refs as R
from oracle import wan_oracle as wo

BF = torch.bfloat16


def _sub_id(sub):
    return "+".join(sub) or "plain"


def _ln_id(c):
    return f"{c[0]}x{c[1]}-{_sub_id(c[2])}"


def _rms_id(c):
    return f"{c[0]}x{c[1]}-hd{c[2]}-t{c[3]}"


# ---------------------------------------------------------------------------------------------------------------------
# a right kernel passes
@pytest.mark.parametrize("case", R.ln_cases(), ids=_ln_id)
def test_layernorm_restatement_passes_both_bars(case):
    rows, dim, sub = case
    x, v = R.ln_inputs(rows, dim, sub)
    chain, m = R.layernorm_chain(x, **v)
    R.assert_pinned(R.layernorm_f32(x, **v), chain, m, f"layernorm f32 {_ln_id(case)}")


@pytest.mark.parametrize("case", R.rms_cases(), ids=_rms_id)
def test_rmsnorm_rope_restatement_passes_both_bars(case):
    rows, dim, hd, scale = case
    x, w, cos, sin = R.rms_inputs(rows, dim, hd, scale)
    chain, m = R.rmsnorm_rope_chain(x, w, cos, sin, hd or 8)
    R.assert_pinned(R.rmsnorm_rope_f32(x, w, cos, sin, hd or 8), chain, m, f"rmsnorm_rope f32 {_rms_id(case)}")


@pytest.mark.parametrize("case", [c for c in R.rms_cases() if c[2] is not None] + [(r, d, h, 1.0) for r, d, h in R.BIG_ROPE], ids=_rms_id)
def test_rope_apply_restatement_passes_both_bars(case):
    rows, dim, hd, scale = case
    x, _, cos, sin = R.rms_inputs(rows, dim, hd, scale)
    chain, m = R.rope_apply_chain(x, cos, sin, hd)
    R.assert_pinned(R.rope_apply_f32(x, cos, sin, hd), chain, m, f"rope_apply f32 {_rms_id(case)}")


def test_the_issue_shapes_stay_far_below_the_cap():
    """515 x 5120, 129 x 1536, 37 x 8192, 72 x 264 for all 16 operand subsets: the restatement differs on at most 6e-5 of the elements.
    These are not inputs of the GPU test; bar (b) is printed per shape, not asserted: at 515 x 5120 (2.6 M elements) the restatement
    itself has 1 to 3 elements outside for the operand sets whose chain rounds more than once (forward_refs.py, bar (b))."""
    worst = 0.0
    for rows, dim in ((515, 5120), (129, 1536), (37, 8192), (72, 264)):
        outside, ratio = 0, 0.0
        for sub in R.SUBSETS:
            x, v = R.ln_inputs(rows, dim, sub)
            chain, m = R.layernorm_chain(x, **v)
            j = R.judge(R.layernorm_f32(x, **v), chain, m)
            assert R.passes(j)[0], (rows, dim, sub, j)
            worst, outside, ratio = max(worst, j["share"]), max(outside, j["outside"]), max(ratio, j["worst"])
        print(f"PIN layernorm f32 {rows}x{dim}, 16 subsets: at most {outside} elements outside 2^-7 m + 2^-16 s, worst {ratio:.2f} of the allowance")
    print(f"PIN layernorm f32, the issue's four shapes x 16 subsets: worst differing share {worst:.2e}")
    assert worst <= R.SHARE_CAP / 7


# ---------------------------------------------------------------------------------------------------------------------
# a subtly wrong kernel does not
def _report(what, fault, j):
    a, b = R.passes(j)
    tripped = " and ".join(n for n, ok in (("(a)", a), ("(b)", b)) if not ok) or "NOTHING"
    print(f"FAULT {what} fault={fault}: trips {tripped} — differing share {j['share']:.2e}, {j['outside']} outside, worst {j['worst']:.2f}x")
    assert not (a and b), f"{what}: fault {fault} passes both bars"
    return a, b


LN_FAULTS = {"dropped_rounding": [("scale1p", "shift"), ("weight", "bias", "scale1p", "shift"), ("scale1p",), ("bias", "shift")],
             "scale_for_1p_scale": [("scale1p", "shift"), ("scale1p",)],
             "mean_drops_last_8": list(R.DIT_SETS)}


@pytest.mark.parametrize("dim", [264, 5120, 8192])
@pytest.mark.parametrize("fault", list(LN_FAULTS))
def test_layernorm_faults_fail_a_bar(fault, dim):
    for sub in LN_FAULTS[fault]:
        x, v = R.ln_inputs(13, dim, sub)
        chain, m = R.layernorm_chain(x, **v)
        assert R.passes(R.judge(R.layernorm_f32(x, **v), chain, m)) == (True, True)
        a, _ = _report(f"layernorm 13x{dim} {_sub_id(sub)}", fault, R.judge(R.layernorm_f32(x, fault=fault, **v), chain, m))
        if fault == "dropped_rounding":
            assert not a, "a dropped rounding is what (a) is for: the per-element allowance alone lets it through"


RMS_FAULT_SHAPES = [(13, 5120, 128, 1.0), (13, 5120, 40, R.Q_PRESCALE_128), (13, 1536, 96, 1.0), (13, 264, 88, 1.0), (13, 8192, 1024, 1.0)]


@pytest.mark.parametrize("case", RMS_FAULT_SHAPES, ids=_rms_id)
@pytest.mark.parametrize("fault", ["dropped_rounding", "mean_drops_last_8", "rope_pair_without_mod", "rope_sin_sign"])
def test_rmsnorm_rope_faults_fail_a_bar(fault, case):
    rows, dim, hd, scale = case
    x, w, cos, sin = R.rms_inputs(rows, dim, hd, scale)
    chain, m = R.rmsnorm_rope_chain(x, w, cos, sin, hd)
    _report(f"rmsnorm_rope {_rms_id(case)}", fault, R.judge(R.rmsnorm_rope_f32(x, w, cos, sin, hd, fault=fault), chain, m))
    if fault.startswith("rope"):
        chain, m = R.rope_apply_chain(x, cos, sin, hd)
        _report(f"rope_apply {_rms_id(case)}", fault, R.judge(R.rope_apply_f32(x, cos, sin, hd, fault=fault), chain, m))


# ---------------------------------------------------------------------------------------------------------------------
# the activations
@pytest.mark.parametrize("kind", ["silu", "gelu_tanh"])
def test_activation_reference_and_restatement(kind):
    """bf16(fp64 function) is the function torch means (fp64 torch agrees where its tanh form does not cancel).  The kernel's formula is
    within one bf16 step of it on EVERY finite input; the naive formula alone is not: in the far negative tail 1 + exp(-z) overflows
    to inf and it returns -0 for a result that is still a normal bf16 number."""
    x = R.all_bf16()
    u = torch.linspace(-5, 12, 3401, dtype=torch.float64)
    fn = torch.nn.functional.silu if kind == "silu" else (lambda t: torch.nn.functional.gelu(t, approximate="tanh"))
    assert float(((fn(u) - R.act_ref(u, kind)).abs() / R.act_ref(u, kind).abs().clamp_min(1e-300)).max()) < 1e-9
    R.assert_act(R.act_f32(x, kind), x, kind, f"act f32 {kind}, all 65536 patterns")
    share, worst = R.act_judge(R.act_naive_f32(x, kind), x, kind)
    print(f"FAULT act {kind} without the tail branch: worst {worst} bf16 steps")
    assert worst > 1
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan")]).to(BF)
    assert torch.equal(R.value_class(R.act_f32(special, kind)), R.value_class(fn(special)))


# ---------------------------------------------------------------------------------------------------------------------
# the chains are the oracle's operations
@pytest.mark.parametrize("rows,dim", [(13, 264), (13, 5120), (37, 1536)])
def test_layernorm_chain_is_the_oracle(rows, dim):
    for sub in R.SUBSETS:
        x, v = R.ln_inputs(rows, dim, sub)
        chain, m = R.layernorm_chain(x, **v)
        ref = wo.layer_norm(x, v["weight"], v["bias"], eps=1e-6)
        if v["scale1p"] is not None:
            ref = ref * v["scale1p"]                # wo.modulate's x * (1 + scale) with the bf16 (1 + scale) already formed
        if v["shift"] is not None:
            ref = ref + v["shift"]
        R.assert_pinned(ref, chain, m, f"oracle layer_norm(+modulate) {rows}x{dim} {_sub_id(sub)}")
    x, v = R.ln_inputs(rows, dim, ("scale1p", "shift"))
    scale = (0.3 * torch.randn(dim, generator=torch.Generator().manual_seed(1))).to(BF)
    chain, m = R.layernorm_chain(x, scale1p=1 + scale, shift=v["shift"])
    R.assert_pinned(wo.modulate(wo.layer_norm(x, eps=1e-6), v["shift"], scale), chain, m, f"oracle modulate(layer_norm) {rows}x{dim}")


@pytest.mark.parametrize("case", [(13, 264, 88, 1.0), (13, 5120, 128, 1.0), (13, 5120, 40, R.Q_PRESCALE_128), (13, 1536, 96, 1.0),
                                  (13, 2048, None, 1.0)], ids=_rms_id)
def test_rmsnorm_rope_chain_is_the_oracle(case):
    rows, dim, hd, scale = case
    x, w, cos, sin = R.rms_inputs(rows, dim, hd, scale)
    chain, m = R.rmsnorm_rope_chain(x, w, cos, sin, hd or 8)
    ref = wo.rms_norm(x, w, 1e-6)
    if hd is not None:
        freqs = torch.complex(cos.double(), sin.double())
        ref = wo.rope_apply(ref[None], freqs, dim // hd)[0]
        ra, _ = R.rope_apply_chain(x, cos, sin, hd)
        want = wo.rope_apply(x[None], freqs, dim // hd)[0]
        assert torch.equal(want.double(), ra), "rope_apply: the oracle is fp64 with one rounding, and so is the chain"
    R.assert_pinned(ref, chain, m, f"oracle rms_norm(+rope_apply) {_rms_id(case)}")


# ---------------------------------------------------------------------------------------------------------------------
# why the wave LayerNorm kernels divide
@pytest.mark.parametrize("dim,exact", [(5120, False), (1536, False), (4096, True)])
def test_a_rounded_reciprocal_of_dim_leaves_a_constant_row_nonzero(dim, exact):
    """x - mean formed as fma(total, fl(-1 / dim), x), emulated in fp64 (the product of two fp32 numbers is exact there) and rounded
    once: 1 / 5120 and 1 / 1536 are not fp32 numbers, so a row of 2.5 keeps d = -2.5 * 1.5e-8, and rstd = 1/sqrt(eps) makes that
    y = -3.7e-5 (-7.5e-5 at 1536) where the chain has exactly 0 — outside both bars, whose allowance is 0 on a row that is 0.  The
    correctly rounded total / dim (what the kernels and the restatement do) leaves 0."""
    c = torch.tensor(2.5, dtype=torch.float32)
    total = c * dim                                                         # exact in fp32
    ninv = torch.tensor(-1.0 / dim, dtype=torch.float32)
    d = (total.double() * ninv.double() + c.double()).float()
    y = d * (1.0 / torch.sqrt(d * d + torch.tensor(1e-6, dtype=torch.float32)))
    print(f"FAULT layernorm mean by a rounded 1/{dim} on a constant row: d = {float(d):.3e}, y = {float(y):.3e}")
    assert (float(d) == 0.0) == exact and float(c - total / dim) == 0.0
    x, v = R.ln_inputs(13, dim, ())
    chain, m = R.layernorm_chain(x, **v)
    row = R.SPECIAL_ROWS["constant"]
    assert not bool(chain[row].any()) and not bool(R.layernorm_f32(x, **v)[row].float().any())
    if not exact:
        got = chain.clone()
        got[row] = float(y)
        assert R.passes(R.judge(got.to(BF), chain, m)) == (False, False)
