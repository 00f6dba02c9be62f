"""The fixed-maximum softmax of kernel 3, modelled on the CPU (attn_fixed_max_cases.model): fp32 scores in the exp2 domain,
p = bf16(exp2(s - m)), fp32 sums over 64-key tiles — with the running maximum and with the maximum fixed at tile 0's row maximum.
What the GPU tests rely on is checked here without a GPU: the two schedules are equally accurate on their inputs, a rise of 90 log2
units stays finite, a rise of 130 and more does not (so the overflow test's input overflows and the others' inputs do not), and a
row whose later tiles all underflow still gives the fp64 answer."""
import pytest
import torch

import attn_fixed_max_cases as fc

BOUND = 2.0 ** -9      # the relative rounding error of one bf16 probability, the only rounding the model has


def _both(q, k, v, h):
    """(fixed error, running error, fixed row sums) of head h against fp64."""
    s = fc.scores(q, k, h).float()
    ref = fc.reference(fc.head(q, h), fc.head(k, h), fc.head(v, h), 1)[0]
    of, lf, _ = fc.model(s, fc.head(v, h), "fixed")
    orun, _, _ = fc.model(s, fc.head(v, h), "running")
    return fc.rel_l2(of, ref), fc.rel_l2(orun, ref), lf, of, ref


@pytest.mark.parametrize("name,sq,skv,heads,std", fc.RANDOM)
def test_fixed_and_running_maximum_are_equally_accurate_on_random_data(name, sq, skv, heads, std):
    """(a) Same level against fp64 on the GPU tests' random inputs.  The model's outputs stay fp32, so the errors are those of the
    bf16 probabilities alone: every p is within 2^-9 of its value, relatively, under either schedule — at any magnitude, bf16
    having fp32's exponent range — so the bar for both is BOUND = 2^-9.  (The running maximum can come out below the fixed one
    on peaky rows: a key that moves the maximum gets p = 1 exactly, with no rounding at all; both figures are printed.)"""
    q, k, v = fc.random_case(1000 + int(std), sq, skv, heads, std)
    ef, er, lf, _, _ = _both(q, k, v, heads - 1)
    print(f"{name}: fixed {ef:.3e}  running {er:.3e}  ratio {ef / er:.3f}")
    assert ef < BOUND and er < BOUND
    assert bool(torch.isfinite(lf).all()) and float(lf.min()) >= 1.0      # the row sum holds the exact term 1


@pytest.mark.parametrize("name,key,rise", fc.RISES)
def test_rises_of_60_and_90_stay_finite_and_accurate(name, key, rise):
    """(a), (b) The inputs of the 'large rise without repair' GPU tests: the rise is what it says, nothing overflows, and the fixed
    maximum is as accurate as the running one on the row the case is built around and on the whole head."""
    q, k, v, got = fc.rise_case(key, rise)
    assert abs(got - rise) < 1.0, got
    ef, er, lf, of, ref = _both(q, k, v, fc.RISE_HEAD)
    row_f = fc.rel_l2(of[fc.RISE_ROW], ref[fc.RISE_ROW])
    print(f"{name}: rise {got:.2f}  fixed {ef:.3e}  running {er:.3e}  row {row_f:.3e}  l[row] {float(lf[fc.RISE_ROW]):.3e}")
    assert bool(torch.isfinite(lf).all()) and bool(torch.isfinite(of).all())
    assert float(lf[fc.RISE_ROW]) > 2.0 ** (rise - 2)
    assert ef < BOUND and er < BOUND and row_f < BOUND


@pytest.mark.parametrize("rise", [130.0, fc.OVERFLOW_RISE, 200.0])
def test_a_rise_of_130_or_more_makes_the_row_sum_non_finite(rise):
    """(c) exp2 of 128 and more is not an fp32 number: the row sum of the fixed-maximum schedule shows it, for that row and for no
    other, while the running maximum handles the same input."""
    q, k, v, got = fc.rise_case(1000, rise)
    assert got >= 129.5
    s = fc.scores(q, k, fc.RISE_HEAD).float()
    _, lf, _ = fc.model(s, fc.head(v, fc.RISE_HEAD), "fixed")
    bad = ~torch.isfinite(lf)
    assert bad.nonzero().flatten().tolist() == [fc.RISE_ROW]
    orun, lr, _ = fc.model(s, fc.head(v, fc.RISE_HEAD), "running")
    ref = fc.reference(fc.head(q, fc.RISE_HEAD), fc.head(k, fc.RISE_HEAD), fc.head(v, fc.RISE_HEAD), 1)[0]
    assert bool(torch.isfinite(lr).all()) and fc.rel_l2(orun, ref) < BOUND


def test_no_other_gpu_case_overflows():
    """(c) The 'zero blocks repaired' assertions of the GPU tests rest on this: every row sum of every other case is finite."""
    cases = [fc.random_case(1000 + int(std), sq, skv, heads, std) + (heads,) for _, sq, skv, heads, std in fc.RANDOM]
    cases += [c() + (2,) for c in (fc.negative_start_case, fc.all_equal_case, fc.huge_then_small_case)]
    for q, k, v, heads in cases:
        for h in range(heads):
            _, lf, _ = fc.model(fc.scores(q, k, h).float(), fc.head(v, h), "fixed")
            assert bool(torch.isfinite(lf).all()) and float(lf.min()) >= 1.0


def test_everything_after_tile_0_underflows_and_the_answer_is_still_right():
    """(d) huge_then_small: row 7's first tile lies ~190 log2 units above every later score; p of every later key is 0 and the
    result is the fp64 answer (whose later terms are below 2^-150 of the sum)."""
    q, k, v = fc.huge_then_small_case()
    s = fc.scores(q, k, 0).float()
    assert float(s[7, :64].max() - s[7, 64:].max()) > 150
    ef, er, lf, of, ref = _both(q, k, v, 0)
    assert float(lf[7]) == 64.0                                   # 64 equal terms of exactly 1, nothing else
    assert fc.rel_l2(of[7], ref[7]) < 1e-6 and ef < BOUND and er < BOUND


def test_negative_first_maximum_and_equal_scores():
    q, k, v = fc.negative_start_case()
    s = fc.scores(q, k, 0).float()
    assert float(s[7, :64].max()) < -30 and float(s[7].max() - s[7, :64].max()) < 90
    ef, er, lf, _, _ = _both(q, k, v, 0)
    assert bool(torch.isfinite(lf).all()) and ef < BOUND and er < BOUND
    q, k, v = fc.all_equal_case()
    ef, er, lf, of, ref = _both(q, k, v, 1)
    assert torch.equal(lf, torch.full_like(lf, 2560.0)) and ef < 1e-5 and er < 1e-5
