"""TeaCache's host side (goal_force_amd/teacache.py): the state machine against the decisions the REFERENCE's own `TeaCache.check`
took inside its `WanVideoPipeline.__call__` (tests/golden/g19_teacache.npz, made by tests/golden/make_teacache_golden.py), and the
three bf16 roundings of the ratio against torch's bf16 arithmetic on the CPU.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import teacache_inputs as ti
from conftest import GOLDEN, ROOT
from goal_force_amd.teacache import COEFFICIENTS, TeaCache, ratio_from_sums

BF = torch.bfloat16
MODEL_IDS = ("Wan2.1-T2V-1.3B", "Wan2.1-T2V-14B", "Wan2.1-I2V-14B-480P", "Wan2.1-I2V-14B-720P")


def _g19():
    return np.load(os.path.join(GOLDEN, "g19_teacache.npz"))


def _cache():
    kw = ti.CALL_KWARGS
    return TeaCache(kw["num_inference_steps"], rel_l1_thresh=kw["tea_cache_l1_thresh"], model_id=kw["tea_cache_model_id"])


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_decide_replays_the_reference_decisions(mode):
    """`decide` fed with the ratios the reference evaluated: the same decision at every one of the 2 x 20 forwards and the same
    accumulated distance after it, as float64 (the same numpy.poly1d on the same Python floats)."""
    g = _g19()
    assert str(g["kwargs_repr"]) == repr(sorted(ti.CALL_KWARGS.items())), "the golden was made with these keyword arguments"
    for branch in range(2):
        tc = _cache()
        for step, (ratio, acc, skip) in enumerate(zip(g[f"ratio_{mode}"][branch], g[f"acc_{mode}"][branch], g[f"skip_{mode}"][branch])):
            forced = step in (0, tc.num_inference_steps - 1)
            assert np.isnan(ratio) == forced
            got = tc.decide(None if forced else float(ratio))
            assert got == bool(skip), (branch, step)
            assert float(tc.accumulated_rel_l1_distance) == float(acc), (branch, step)
    assert 5 <= int(g[f"skip_{mode}"][0].sum()) <= 15


def test_step_counter_wraps_a_second_pass_reproduces_the_first():
    g = _g19()
    tc = _cache()
    ratios = g["ratio_bf16"][0]
    passes = []
    for _ in range(2):
        assert tc.step == 0
        passes.append([(tc.decide(None if np.isnan(r) else float(r)), float(tc.accumulated_rel_l1_distance)) for r in ratios])
    assert passes[0] == passes[1] and [s for s, _ in passes[0]] == [bool(s) for s in g["skip_bf16"][0]]


def _pair(n, seed):
    """A t_mod-like pair: prev ~ offset + noise, cur = prev + a perturbation of seeded relative size (1e-3 .. 1)."""
    g = torch.Generator().manual_seed(seed)
    prev = (torch.randn(n, generator=g) * (1 + seed % 7)).to(BF)
    rel = 10.0 ** (-3 * float(torch.rand((), generator=g)))
    cur = (prev.float() + rel * torch.randn(n, generator=g) * (1 + seed % 7)).to(BF)
    return cur, prev


def _off_boundary(mean64):
    """True if the value is further than 1e-4 relative from every bf16 rounding boundary (the midpoints between neighbouring bf16
    values): there an fp32 and an fp64 evaluation of the mean round to the same bf16."""
    m, e = np.frexp(mean64)                     # mean64 = m * 2^e, m in [0.5, 1): bf16 has 8 significant bits -> spacing 2^-8 in m
    frac = (m * 256.0) % 1.0                    # position between two neighbouring bf16 values
    return abs(frac - 0.5) * (2.0 ** -8) / m > 1e-4


@pytest.mark.parametrize("n", [1536, 30720])
def test_ratio_from_sums_is_torch_bf16_arithmetic(n):
    """`ratio_from_sums` on fp64 sums of the bf16-rounded terms == `((a - b).abs().mean() / b.abs().mean()).item()` on CPU bf16 tensors,
    exactly, on 200 seeded pairs whose two means sit off every bf16 rounding boundary (asserted: a precondition on the inputs)."""
    checked, seed = 0, 0
    while checked < 200:
        seed += 1
        assert seed < 2000, "the draw keeps landing on rounding boundaries"
        cur, prev = _pair(n, seed * 2 + (n == 30720))
        s_diff = float((cur - prev).abs().double().sum())          # (cur - prev) is torch's bf16 subtraction: one rounding per element
        s_prev = float(prev.abs().double().sum())
        if not (_off_boundary(s_diff / n) and _off_boundary(s_prev / n)):
            continue
        assert _off_boundary(s_diff / n) and _off_boundary(s_prev / n)
        want = ((cur - prev).abs().mean() / prev.abs().mean()).item()
        assert ratio_from_sums(s_diff, s_prev, n) == want, (seed, s_diff, s_prev, want)
        checked += 1


def test_ratio_from_sums_with_a_zero_previous_does_not_raise():
    assert np.isinf(ratio_from_sums(3.0, 0.0, 8)) and np.isnan(ratio_from_sums(0.0, 0.0, 8))


def test_unknown_model_id_names_the_four_supported_ones():
    with pytest.raises(ValueError) as e:
        TeaCache(20, rel_l1_thresh=0.26, model_id="Wan2.2-I2V-A14B")
    assert all(m in str(e.value) for m in MODEL_IDS) and "Wan2.2-I2V-A14B" in str(e.value)
    assert tuple(COEFFICIENTS) == MODEL_IDS and all(len(c) == 5 for c in COEFFICIENTS.values())
    tc = _cache()
    for name in ("num_inference_steps", "step", "accumulated_rel_l1_distance", "previous_modulated_input", "rel_l1_thresh",
                 "previous_residual", "previous_hidden_states", "coefficients"):      # the reference's attribute names
        assert hasattr(tc, name), name


def test_pipeline_validates_the_model_id_before_any_work():
    from goal_force_amd.pipeline import TeaCache as exported, WanVideoPipeline
    assert exported is TeaCache
    pipe = object.__new__(WanVideoPipeline)            # no modules: the refusal must come before anything is touched
    with pytest.raises(ValueError, match="not a supported TeaCache model id"):
        WanVideoPipeline.__call__(pipe, tea_cache_l1_thresh=0.1, tea_cache_model_id="nope")


def test_header_declares_the_two_kernels_and_the_abi_revision_stays():
    hdr = open(os.path.join(ROOT, "include", "goalforce.h")).read()
    from goal_force_amd import _lib
    for s in ("gf_rel_l1_bf16", "gf_sub_bf16"):
        assert re.search(r"GF_API\s+int\s+" + s + r"\(", hdr), s
        assert s in _lib.SYMBOLS
    lib = _lib.load()
    assert _lib.ABI_VERSION == 20 and lib.gf_abi_version() == 20
    assert hasattr(lib, "gf_rel_l1_bf16") and hasattr(lib, "gf_sub_bf16")
