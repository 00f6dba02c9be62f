"""Sliding-window sampling, the parts that need no GPU: the torch restatement of the temporal tiler (tests/sliding_window_refs.py)
against what the REFERENCE's own TemporalTiler_BCTHW returned (tests/golden/g20_sliding_window.npz part (a)), bit for bit; the
restatement's mask against the reference's vector expression; four injected faults; the argument refusals; the C ABI declarations."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import gen_inputs as gi
import sliding_window_refs as sw
from conftest import GOLDEN, ROOT

BF = torch.bfloat16


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "g20_sliding_window.npz"))


def _case(g, T, size, stride):
    k = sw.case_key(T, size, stride)
    wins = gi.from_u16(g[f"a_{k}_windows"])
    outs, at = [], 0
    for t, t_ in sw.windows(T, size, stride):
        outs.append(wins[:, :, at:at + t_ - t])
        at += t_ - t
    assert at == wins.shape[2]
    return gi.from_u16(g[f"a_{k}_latents"]), gi.from_u16(g[f"a_{k}_y"]), outs, gi.from_u16(g[f"a_{k}_value"])


@pytest.mark.parametrize("T,size,stride", sw.TILER_CASES)
def test_restatement_equals_the_reference_tiler_bit_for_bit(golden, T, size, stride):
    latents, y, want_outs, want = _case(golden, T, size, stride)
    lat2, y2 = sw.tiler_inputs(T)
    assert torch.equal(lat2, latents) and torch.equal(y2, y), "the seeded inputs are not the golden's"
    outs, value = sw.run(sw.toy_model_fn, size, stride, latents, y)
    assert len(outs) == len(want_outs) and all(torch.equal(a, b) for a, b in zip(outs, want_outs))
    assert value.dtype == BF and torch.equal(value, want)
    assert torch.equal(sw.blend(want_outs, T, size, stride), want)


def test_schedule_of_the_cases():
    """What the table of cases is there to cover."""
    assert sw.windows(5, 8, 4) == [(0, 5)]                                     # one window
    assert sw.windows(25, 21, 10) == [(0, 21), (10, 25)]                       # short last window, no window at t = 20
    assert sw.windows(7, 3, 3) == [(0, 3), (3, 6), (6, 7)]                     # border 0
    assert sw.windows(5, 3, 1) == [(0, 3), (1, 4), (2, 5)]                     # the middle window has both ramps, overlapping
    assert sw.windows(6, 4, 1) == [(0, 4), (1, 5), (2, 6)]                     # ... and here they overlap off the centre
    assert not torch.equal(sw.mask_1d(4, False, False, 3), sw.mask_1d(4, False, False, 3, fault="left_ramp_last"))
    assert torch.equal(sw.mask_1d(3, False, False, 2), sw.mask_1d(3, False, False, 2, fault="left_ramp_last"))
    assert sw.windows(41, 21, 10) == [(0, 21), (10, 31), (20, 41)] and sw.windows(41, 21, 20) == [(0, 21), (20, 41)]
    for T, size, stride in sw.TILER_CASES:                                     # every ramped window is longer than its border
        for t, t_ in sw.windows(T, size, stride):
            assert (t == 0 and t_ == T) or t_ - t > size - stride
    from goal_force_amd.temporal_tiler import TemporalTiler_BCTHW
    for T in range(1, 45):
        for size in range(1, 24):
            for stride in range(1, size + 1):
                assert TemporalTiler_BCTHW.windows(T, size, stride) == sw.windows(T, size, stride)


def _vector_mask(n, left_bound, right_bound, border):
    """The reference's expression: whole ramps assigned to the two ends of a vector of ones, the right end last."""
    x = torch.ones((n,))
    if border == 0:
        return x
    ramp = (torch.arange(border) + 0.5) / border
    if not left_bound:
        x[:border] = ramp
    if not right_bound:
        x[-border:] = torch.flip(ramp, dims=(0,))
    return x


def test_mask_bits_equal_the_vector_expression_for_every_border_and_position():
    checked = 0
    for border in range(1, 41):
        for n in sorted({border, border + 1, 2 * border - 1, 2 * border, 2 * border + 1, 41, 64}):      # len < 2*border among them
            if n < border:
                continue
            for lb in (False, True):
                for rb in (False, True):
                    want, got = _vector_mask(n, lb, rb, border), sw.mask_1d(n, lb, rb, border)
                    assert got.dtype == torch.float32 and torch.equal(got, want), (border, n, lb, rb)
                    assert torch.equal(got.to(BF), want.to(BF))
                    checked += n
    assert torch.equal(sw.mask_1d(5, False, False, 0), torch.ones(5))
    assert checked > 10000


@pytest.mark.parametrize("fault,case", [("left_ramp_last", (6, 4, 1)),("shift_one", (11, 5, 2)), ("one_rounding", (41, 21, 10)),
                                        ("descending", (5, 3, 1))])
def test_an_injected_fault_breaks_the_equality(golden, fault, case):
    """The restatement is not vacuous: each of these deviations changes the bits of the named case."""
    assert fault in sw.FAULTS
    _, _, outs, want = _case(golden, *case)
    assert torch.equal(sw.blend(outs, *case), want)
    assert not torch.equal(sw.blend(outs, *case, fault=fault), want), f"{fault} goes unnoticed on {case}"


def test_tiler_refuses_by_name():
    from goal_force_amd._lib import GoalForceError
    from goal_force_amd.temporal_tiler import TemporalTiler_BCTHW, check_window
    kw = dict(latents=torch.zeros((1, 2, 5, 2, 3), dtype=BF))

    def run(size, stride, **more):
        return TemporalTiler_BCTHW().run(lambda **k: None, size, stride, "cuda", BF, model_kwargs=dict(kw),
                                         tensor_names=["latents", "y"], **more)
    for size, stride, msg in ((3, 4, "exceeds sliding_window_size"), (0, 0, "must be positive"), (3, 0, "must be positive"),
                              (-2, -3, "must be positive"), (3, -1, "must be positive"), (3.0, 2, "must be an integer"),
                              (3, 2.5, "must be an integer"), (True, 1, "must be an integer"), ("3", 2, "must be an integer"),
                              (3, None, "must be given together"), (None, 2, "must be given together")):
        with pytest.raises(GoalForceError, match=msg):
            run(size, stride)
        with pytest.raises(GoalForceError, match=msg):
            check_window(size, stride)
    assert check_window(None, None) is None and check_window(3, 3) == (3, 3) and check_window(21, 10) == (21, 10)
    for bs in (2, 0, 3):
        with pytest.raises(GoalForceError, match="batch_size"):
            run(3, 2, batch_size=bs)
    with pytest.raises(GoalForceError, match="no CPU fallback"):         # batch_size None and 1 pass that check (CPU tensors do not)
        run(3, 2, batch_size=None)
    with pytest.raises(GoalForceError, match="no CPU fallback"):
        run(3, 2, batch_size=1)
    import inspect
    names = list(inspect.signature(TemporalTiler_BCTHW.run).parameters)
    assert names[:9] == ["self", "model_fn", "sliding_window_size", "sliding_window_stride", "computation_device",
                         "computation_dtype", "model_kwargs", "tensor_names", "batch_size"]     # the reference's signature (B3)


def test_model_fn_and_pipeline_refuse_half_a_window_before_any_work():
    from goal_force_amd._lib import GoalForceError
    from goal_force_amd.model_fn import model_fn_wan_video
    from goal_force_amd.pipeline import TemporalTiler_BCTHW, WanVideoPipeline
    from goal_force_amd import temporal_tiler
    assert TemporalTiler_BCTHW is temporal_tiler.TemporalTiler_BCTHW
    dit = types.SimpleNamespace(require_clip_embedding=False)
    for kw in (dict(sliding_window_size=3), dict(sliding_window_stride=2)):
        with pytest.raises(GoalForceError, match="must be given together"):
            model_fn_wan_video(dit, **kw)
        pipe = object.__new__(WanVideoPipeline)            # no modules: the refusal must come before anything is touched
        with pytest.raises(GoalForceError, match="must be given together"):
            WanVideoPipeline.__call__(pipe, **kw)
        with pytest.raises(GoalForceError, match="must be given together"):
            WanVideoPipeline.denoise(pipe, None, None, None, None, None, **kw)
    with pytest.raises(GoalForceError, match="exceeds sliding_window_size"):
        model_fn_wan_video(dit, sliding_window_size=2, sliding_window_stride=3)
    with pytest.raises(NotImplementedError, match="cfg_merge"):          # stays refused
        WanVideoPipeline.__call__(object.__new__(WanVideoPipeline), cfg_merge=True, sliding_window_size=3, sliding_window_stride=2)


def test_header_declares_the_two_entry_points_and_the_abi_revision_stays():
    hdr = open(os.path.join(ROOT, "include", "goalforce.h")).read()
    from goal_force_amd import _lib, ops
    i, i64, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    for s in ("gf_window_blend", "gf_window_finalize"):
        assert re.search(r"GF_API\s+int\s+" + s + r"\(", hdr), s
        assert s in _lib.SYMBOLS
    assert _lib.BINDINGS["gf_window_blend"] == (i, [p, p, p, i64, i64, i64, i64, i64, i64, i64, i, i, i64, p])
    assert _lib.BINDINGS["gf_window_finalize"] == (i, [p, p, i64, i64, i64, i64, i64, p])
    lib = _lib.load()
    assert _lib.ABI_VERSION == 20 and lib.gf_abi_version() == 20
    assert hasattr(lib, "gf_window_blend") and hasattr(lib, "gf_window_finalize")
    assert callable(ops.window_blend) and callable(ops.window_finalize)
    # the header spells the arithmetic out
    text = " ".join(hdr.split())
    for phrase in ("fp32(i + 0.5) / fp32(border)", "fp32(len - 1 - i + 0.5) / fp32(border)", "wins where both apply"):
        assert phrase in text, phrase
