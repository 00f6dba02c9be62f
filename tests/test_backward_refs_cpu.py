"""The checker of the backward-kernel tests, checked on the CPU (no GPU needed).

tests/test_backward_kernels_gpu.py holds gf_backward.hip against the fp64 references of tests/backward_refs.py through one per-element
bound.  This file is the evidence that those tests mean something:
 (a) an fp32 restatement of every kernel's chain — the same formulas, another summation order — stays inside the bound at the shapes the
     GPU tests use, so a right kernel passes;
 (b) four plausible kernel faults injected into the restatements at dim = 5120 land outside it — and the first of them (a row mean that
     misses one 16-byte chunk) is shown to pass the 6e-3 rel-L2 bar the suite used before, which is why the bound is per element.
"""
import pytest
import torch

import backward_refs as R

BF = torch.bfloat16
WAVE_DIMS = (8, 256, 512, 520, 1536, 5112, 5120)
BLOCK_DIMS = (8, 1024, 1032, 1536, 5120, 8192, 5128)
DIMS = sorted(set(WAVE_DIMS + BLOCK_DIMS))


def _hd(dim):
    return 128 if dim % 128 == 0 else 64 if dim % 64 == 0 else 8


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------
# (a) the restatements are inside the bound
@pytest.mark.parametrize("gmode", ["none", "affine", "scale1p"])
@pytest.mark.parametrize("dim", DIMS)
def test_layernorm_bwd_restatement_is_inside_the_bound(dim, gmode):
    for rows in (1, 37):
        x, dy, g = R.row_inputs(rows, dim, _gen(dim + rows), gmode)
        if rows == 37:
            x[5] = 2.5                                                  # variance 0: rstd = eps^-1/2
        dx_ref, dg_ref, db_ref = R.layernorm_bwd_ref(x, dy, g)
        dx, dg, db = R.layernorm_bwd_f32(x, dy, g)
        R.assert_within(dx, dx_ref, R.row_rms(dx_ref), f"layernorm_bwd f32 ({rows}, {dim}) g={gmode}")
        if rows > 1:
            assert R.rel_l2(dg, dg_ref) <= 2e-3 and R.rel_l2(db, db_ref) <= 1e-5


@pytest.mark.parametrize("rope", ["none", "unit", "prescaled"])
@pytest.mark.parametrize("dim", DIMS)
def test_rmsnorm_rope_bwd_restatement_is_inside_the_bound(dim, rope):
    hd = _hd(dim)
    for rows in (1, 37):
        gen = _gen(3 * dim + rows)
        x, dy, w = R.row_inputs(rows, dim, gen, "affine")
        if rows == 37:
            x[7] = 0.0                                                  # rstd = eps^-1/2, xn = 0
        cos, sin = (None, None) if rope == "none" else R.rope_table(rows, hd, gen, 1.0 if rope == "unit" else 0.1275)
        dx_ref, dw_ref = R.rmsnorm_rope_bwd_ref(x, dy, w, cos, sin, hd)
        dx, dw = R.rmsnorm_rope_bwd_f32(x, dy, w, cos, sin, hd)
        R.assert_within(dx, dx_ref, R.row_rms(dx_ref), f"rmsnorm_rope_bwd f32 ({rows}, {dim}) hd={hd} rope={rope}")
        if rows > 1:
            assert R.rel_l2(dw, dw_ref) <= 2e-3


def test_the_issue_shapes_have_zero_violations():
    """(37, 5120), (75, 256), (41, 1544): the shapes the bound was first checked at."""
    for rows, dim in ((37, 5120), (75, 256), (41, 1544)):
        gen = _gen(rows)
        x, dy, g = R.row_inputs(rows, dim, gen, "scale1p")
        ref = R.layernorm_bwd_ref(x, dy, g)[0]
        assert R.violations(R.layernorm_bwd_f32(x, dy, g)[0], ref, R.row_rms(ref))[0] == 0
        cos, sin = R.rope_table(rows, 8, gen)
        ref = R.rmsnorm_rope_bwd_ref(x, dy, g, cos, sin, 8)[0]
        assert R.violations(R.rmsnorm_rope_bwd_f32(x, dy, g, cos, sin, 8)[0], ref, R.row_rms(ref))[0] == 0


@pytest.mark.parametrize("kind", ["gelu_tanh", "silu"])
def test_act_bwd_restatement_is_inside_the_bound(kind):
    for n in (8, 4104, 66560, 200000):
        u, df = R.act_inputs(n, _gen(n))
        ref = R.act_bwd_ref(u, df, kind)
        assert bool(torch.isfinite(ref).all())
        R.assert_within(R.act_bwd_f32(u, df, kind), ref, df.double().abs(), f"act_bwd f32 {kind} n={n}")
    # the closed form is the derivative: fp64 autograd of torch's own activation agrees
    u = torch.linspace(-12, 12, 4001, dtype=torch.float64)
    with torch.enable_grad():
        ud = u.clone().requires_grad_(True)
        fn = (lambda t: torch.nn.functional.gelu(t, approximate="tanh")) if kind == "gelu_tanh" else torch.nn.functional.silu
        fn(ud).sum().backward()
    assert float((ud.grad - R.act_grad_ref(u, kind)).abs().max()) < 1e-12


def test_mse_sumsq_colsum_restatements():
    for n in (8, 1003, 300007):
        for weight in (1.0, 0.37):
            g = _gen(n)
            p, t = torch.randn((n,), generator=g).to(BF), torch.randn((n,), generator=g).to(BF)
            loss_ref, grad_ref = R.mse_ref(p, t, weight)
            loss, grad = R.mse_f32(p, t, weight)
            assert abs(loss - loss_ref) <= 1e-5 * loss_ref
            R.assert_within(grad, grad_ref, grad_ref.abs(), f"mse grad f32 n={n} weight={weight}")
    for n in (1, 1003, 600011):
        x = torch.randn((n,), generator=_gen(n)).to(BF)
        assert abs(R.sumsq_f32(x) - R.sumsq_ref(x)) <= 1e-5 * R.sumsq_ref(x)
    for rows, cols in ((1, 8), (65, 2056), (4100, 512)):
        g = _gen(rows)
        a, b = torch.randn((rows, cols), generator=g).to(BF), torch.randn((rows, cols), generator=g).to(BF)
        assert R.rel_l2(R.colsum_f32(a), R.colsum_ref(a)) <= 1e-5 and R.rel_l2(R.colsum_f32(a, b), R.colsum_ref(a, b)) <= 1e-5


@pytest.mark.parametrize("case", R.ADAMW_CASES, ids=R.adamw_id)
def test_adamw_restatement_and_a_wrong_grad_scale(case):
    kw = {k: v for k, v in case.items() if k != "moments"}
    p, gr, m, v = R.adamw_state(1003, case["moments"], 7)
    ref = R.adamw_ref(p, gr, m, v, lr=1e-2, **kw)
    got = R.adamw_f32(p, gr, m, v, lr=1e-2, **kw)
    R.adamw_check(*got, ref, f"adamw f32 {case}")
    if case["grad_scale"] != 1.0:                                       # a kernel that ignored grad_scale: only the moments show it
        wrong = R.adamw_f32(p, gr, m, v, lr=1e-2, **{**kw, "grad_scale": 1.0})
        assert R.rel_l2(wrong[1], ref[1]) > 1e-5 and R.rel_l2(wrong[2], ref[2]) > 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# (b) injected faults are outside it at the shipped width
def test_a_row_mean_that_misses_its_last_chunk_is_caught_by_the_bound_and_not_by_rel_l2():
    rows, dim = 37, 5120
    for gmode in ("none", "scale1p"):
        x, dy, g = R.row_inputs(rows, dim, _gen(11), gmode)
        ref = R.layernorm_bwd_ref(x, dy, g)[0]
        good, bad = R.layernorm_bwd_f32(x, dy, g)[0], R.layernorm_bwd_f32(x, dy, g, fault="mean_drops_last_8")[0]
        n_bad = R.violations(bad, ref, R.row_rms(ref))[0]
        print(f"layernorm g={gmode}: rel-L2 good {R.rel_l2(good, ref):.3e} faulty {R.rel_l2(bad, ref):.3e}; "
              f"faulty outside the bound on {n_bad / ref.numel():.1%} of the elements; good/floor {R.floor_ratio(good, ref):.3f}")
        assert R.violations(good, ref, R.row_rms(ref))[0] == 0
        assert n_bad > 0.01 * ref.numel()
        assert R.rel_l2(bad, ref) < 6e-3, "the old bar was expected to miss this fault: that is the point of the per-element bound"
    x, dy, w = R.row_inputs(rows, dim, _gen(12), "affine")
    cos, sin = R.rope_table(rows, 128, _gen(13))
    ref = R.rmsnorm_rope_bwd_ref(x, dy, w, cos, sin, 128)[0]
    bad = R.rmsnorm_rope_bwd_f32(x, dy, w, cos, sin, 128, fault="mean_drops_last_8")[0]
    assert R.violations(bad, ref, R.row_rms(ref))[0] > 0


def test_rope_inverse_with_the_wrong_sign_of_sin_is_caught():
    x, dy, w = R.row_inputs(37, 5120, _gen(14), "affine")
    for scale in (1.0, 0.1275):
        cos, sin = R.rope_table(37, 128, _gen(15), scale)
        dx_ref, dw_ref = R.rmsnorm_rope_bwd_ref(x, dy, w, cos, sin, 128)
        dx, dw = R.rmsnorm_rope_bwd_f32(x, dy, w, cos, sin, 128, fault="rope_sin_sign")
        assert R.violations(dx, dx_ref, R.row_rms(dx_ref))[0] > 0.5 * dx.numel() and R.rel_l2(dw, dw_ref) > 2e-3


def test_one_plus_scale_taken_as_scale_is_caught():
    x, dy, g = R.row_inputs(37, 5120, _gen(16), "scale1p")
    ref = R.layernorm_bwd_ref(x, dy, g)[0]
    bad = R.layernorm_bwd_f32(x, dy, g, fault="scale_for_1p_scale")[0]
    assert R.violations(bad, ref, R.row_rms(ref))[0] > 0.5 * ref.numel()


def test_dz_times_w_before_the_dw_product_is_caught():
    x, dy, w = R.row_inputs(37, 5120, _gen(17), "affine")
    cos, sin = R.rope_table(37, 128, _gen(18))
    dx_ref, dw_ref = R.rmsnorm_rope_bwd_ref(x, dy, w, cos, sin, 128)
    dx, dw = R.rmsnorm_rope_bwd_f32(x, dy, w, cos, sin, 128, fault="dw_after_weight")
    assert R.violations(dx, dx_ref, R.row_rms(dx_ref))[0] == 0          # dx is untouched by this fault: only dw shows it
    assert R.rel_l2(dw, dw_ref) > 2e-3
    assert R.rel_l2(R.rmsnorm_rope_bwd_f32(x, dy, w, cos, sin, 128)[1], dw_ref) <= 2e-3
