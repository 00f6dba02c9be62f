"""The coherence gate of the mass-cover maps, everything that needs no GPU: the fp64 restatement (tests/coherence_refs.py) on hand-made
rows, the sensitivity of the GPU tests' bound and of their exact selection to the mistakes they are there to catch, the fp64
conditions of the guarantee test, the Python layer's argument errors and the C ABI's declarations."""
import ctypes
import os
import re

import pytest
import torch

import adaptive_map_refs as ar
import coherence_refs as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATED_SYMBOLS = ("gf_block_map_gated_workspace_bytes", "gf_block_means_coh", "gf_block_map_select_gated", "gf_block_map_from_qk_gated")
NAN, INF = float("nan"), float("inf")


def hand_rows(kind, n, seed=0):
    """[n, 128] fp64 rows of one data class."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(128, generator=g, dtype=torch.float64)
    if kind == "equal":
        return v.repeat(n, 1)
    if kind == "zero":
        return torch.zeros((n, 128), dtype=torch.float64)
    if kind == "halves":
        return torch.cat([v.repeat(n // 2, 1), -v.repeat(n // 2, 1)])
    if kind == "onehot":
        return 3.0 * torch.eye(128, dtype=torch.float64)[:n]
    if kind == "std1":
        return torch.randn((n, 128), generator=g, dtype=torch.float64)
    if kind == "offset":
        return torch.randn((n, 128), generator=g, dtype=torch.float64) + 4.0
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------ the restatement, in closed form
def test_coherence_of_the_data_classes_in_closed_form():
    for n in (2, 16, 64):
        assert cr.coherence(hand_rows("equal", n), 1, 64).tolist() == [[pytest.approx(1.0, abs=1e-14)]]
        assert cr.coherence(hand_rows("zero", n), 1, 64).tolist() == [[1.0]]                      # by definition
        assert cr.coherence(hand_rows("halves", n), 1, 64).tolist() == [[pytest.approx(0.0, abs=1e-28)]]
        assert cr.coherence(hand_rows("onehot", n), 1, 64).tolist() == [[pytest.approx(1.0 / n, abs=1e-15)]]
    # std 1: E rho = 1 / n (+ O(1 / (128 n))); std 1 + offset 4: |m|^2 ~ 16 d + d / n, e ~ 17 d
    assert float(cr.coherence(hand_rows("std1", 64), 1, 64)) == pytest.approx(1 / 64, rel=0.25)
    assert float(cr.coherence(hand_rows("offset", 64), 1, 64)) == pytest.approx((16 + 1 / 64) / 17, rel=0.03)
    # 0 <= rho <= 1, per head and per run; a ragged last run uses its own count
    x = torch.cat([hand_rows("equal", 64), hand_rows("onehot", 6)]).repeat(1, 2)
    x[:, 128:] = hand_rows("std1", 70, seed=3)
    rho = cr.coherence(x, 2, 64)
    assert rho.shape == (2, 2) and bool(((rho >= 0) & (rho <= 1 + 1e-14)).all())
    assert float(rho[0, 0]) == pytest.approx(1.0) and float(rho[0, 1]) == pytest.approx(1 / 6)


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_non_finite_rows_give_a_nan_coherence_and_leave_the_other_runs_and_heads_alone(bad):
    x = hand_rows("std1", 130).repeat(1, 2)
    x[70, 128 + 5] = bad
    rho = cr.coherence(x, 2, 64)
    assert torch.isnan(rho).tolist() == [[False, False, False], [False, True, False]]


# --------------------------------------------------------------------------------- the bound would catch the mistakes it is for
def _variants(x, block):
    """rho of one head's [rows, 128] under three wrong recipes, fp64 [n_blocks] each."""
    div, swapped, rounded = [], [], []
    for r0 in range(0, x.shape[0], block):
        run = x[r0: r0 + block]
        n = run.shape[0]
        e = (run * run).sum(1).mean()
        m = run.mean(0)
        div.append((run.sum(0) / block).square().sum() / ((run * run).sum() / block))          # a ragged run divided by the block size
        swapped.append(e / m.square().sum() if float(m.square().sum()) else torch.tensor(1.0, dtype=torch.float64))
        rounded.append(m.to(cr.BF).double().square().sum() / e)                                # the energy of the bf16-rounded mean
        assert n <= block
    return torch.stack(div), torch.stack(swapped), torch.stack(rounded)


@pytest.mark.parametrize("block", [64, 256])
def test_the_coherence_bound_separates_the_wrong_recipes(block):
    bound = cr.coherence_bound(block)
    assert bound < 2.0 ** -15                                            # the derivation lands below the issue's own estimate
    assert cr.coherence_bound(256) == pytest.approx(191 * 2.0 ** -24, rel=2e-3) and cr.coherence_bound(64) == pytest.approx(71 * 2.0 ** -24, rel=2e-3)
    rows = block + 17                                                    # a ragged last run of 17 rows
    caught = {"div": False, "swapped": False, "rounded": False}
    for kind in ("equal", "onehot", "std1", "offset"):
        x = hand_rows(kind, 128, seed=2).repeat(-(-rows // 128), 1)[:rows] if kind in ("equal", "onehot") else hand_rows(kind, rows, seed=2)
        x = x.to(cr.BF).double()
        ref = cr.coherence(x, 1, block)[0]
        for name, got in zip(caught, _variants(x, block)):
            caught[name] = caught[name] or float((got - ref).abs().max()) > bound
    assert all(caught.values()), caught
    # and each on the class that shows it most plainly
    x = hand_rows("offset", rows, seed=4).to(cr.BF).double()
    ref = cr.coherence(x, 1, block)[0]
    div, swapped, rounded = _variants(x, block)
    assert abs(float(div[-1] - ref[-1])) > 0.5                           # 17 / block of the true value
    assert float((swapped - ref).abs().min()) > 0.05
    assert float((rounded - ref).abs().max()) > bound


# ----------------------------------------------------------------------------- the gated selection on hand-made rows and item 2
def test_gated_selection_on_hand_made_rows():
    s = torch.tensor([[[3.0, 2.0, 1.0, 0.0, 0.0]]], dtype=torch.float64)            # w = 8, 4, 2, 1, 1 (W = 16)
    one = torch.ones((1, 1), dtype=torch.float32)
    sel = lambda **kw: cr.select_gated(s, 0.5, **kw)[0, 0].tolist()                  # noqa: E731
    assert sel() == [True, True, False, False, False] == ar.select(s, 0.5)[0, 0].tolist()
    # the query gate: below the threshold and NaN fire, equality passes
    assert sel(q_coh=one * 0.75, q_min=0.75) == [True, True, False, False, False]
    assert sel(q_coh=one * cr.BELOW, q_min=0.75) == [True] * 5
    assert sel(q_coh=one * NAN, q_min=0.75) == [True] * 5
    # the key gate: a fired tile is forced and counts in F — tile 3 (w = 1) forced: 1 + 8 >= 8; tile 0 forced alone holds the mass: floor
    k = torch.ones((1, 5), dtype=torch.float32)
    k[0, 3] = 0.2
    assert sel(k_coh=k, k_min=0.75) == [True, False, False, True, False]
    k[0, 3], k[0, 0] = 1.0, NAN
    assert sel(k_coh=k, k_min=0.75) == [True, True, False, False, False]
    k[0, 0], k[0, 4] = 0.75, cr.BELOW
    forced = torch.tensor([[False, False, True, False, False]])
    assert sel(k_coh=k, k_min=0.75, forced=forced) == [True, False, True, False, True]          # F = 2 + 1, + 8 >= 8
    assert cr.kept_gated(s, cr.select_gated(s, 0.5, q_coh=one * 0.1, q_min=0.75)).tolist() == [[1.0]]


@pytest.mark.parametrize("with_forced", [False, True])
@pytest.mark.parametrize("n_t", [2, 31, 32, 33, 64, 65, 1023, 1024])
def test_item_2_case_has_what_it_is_for(n_t, with_forced):
    """The GPU test's case at every n_t: per-head coherences matter, `>` in place of `>=` changes the selection, the gate-forced tiles
    alone reach the mass somewhere and (without shared forced bits) the two-tile floor is needed."""
    s, forced, q_coh, k_coh = cr.gate_case(n_t, with_forced)
    for tau in (0.5, 0.75):
        want = cr.select_gated(s, tau, forced, q_coh, k_coh, cr.GATE_MIN, cr.GATE_MIN)
        assert bool((want.sum(2) >= 2).all())
        # query-gated rows: everything; at the threshold: not gated
        assert bool(want[0, 2].all() and want[0, 3].all() and want[1, 0].all() and want[2, 1].all())
        if n_t > 2:
            assert not bool(want[0, 1].all()) and not bool(want[1, 3].all()) and not bool(want[2, 0].all())
        # `>`: equality fires too
        gt = lambda c: torch.where(c == cr.GATE_MIN, torch.full_like(c, cr.BELOW), c)          # noqa: E731
        if n_t == 2:
            assert bool(want.all())                                      # two tiles: the floor alone selects both
            continue
        assert not torch.equal(cr.select_gated(s, tau, forced, gt(q_coh), k_coh, cr.GATE_MIN, cr.GATE_MIN), want)
        if n_t >= 31:
            assert not torch.equal(cr.select_gated(s, tau, forced, q_coh, gt(k_coh), cr.GATE_MIN, cr.GATE_MIN), want)
        # head 0's coherences for every head
        assert not torch.equal(cr.select_gated(s, tau, forced, q_coh[:1].expand(3, -1), k_coh, cr.GATE_MIN, cr.GATE_MIN), want)
        if n_t >= 31:
            assert not torch.equal(cr.select_gated(s, tau, forced, q_coh, k_coh[:1].expand(3, -1), cr.GATE_MIN, cr.GATE_MIN), want)
        # the gate changes something against the ungated selection, on both sides
        assert not torch.equal(cr.select_gated(s, tau, forced, None, k_coh, None, cr.GATE_MIN), ar.select(s, tau, forced))
        # head 1, block 2: its one fired tile is the dominant one — the gate-forced tile alone reaches mass W; the floor adds the second
        w, W = ar.weights(s[1, 2])
        fired = ~cr._passes(k_coh[1], cr.GATE_MIN)
        assert int(fired.sum()) == 1 and float(w[fired].sum()) >= tau * float(W) and bool(want[1, 2][fired].all())
        if not with_forced:
            assert int(want[1, 2].sum()) == 2


# ---------------------------------------------------------------------------------------- the guarantee's conditions in fp64
@pytest.mark.parametrize("heads", [2, 3])
@pytest.mark.parametrize("runs", cr.GUARANTEE_RUNS)
def test_item_5_conditions_hold_in_fp64(runs, heads):
    q, k, _ = cr.guarantee_operands(*runs, heads)
    tau, bar = cr.GUARANTEE_MASS, cr.GUARANTEE_MASS * (1 - 2.0 ** -7)
    plain, q_coh, k_coh = cr.map_fp64(q, k, heads, tau, cr.LN2)
    gated, _, _ = cr.map_fp64(q, k, heads, tau, cr.LN2, cr.GUARANTEE_MIN, cr.GUARANTEE_MIN)
    lo_plain = float(cr.retained_fp64(q, k, heads, plain, cr.LN2).min())
    lo_gated = float(cr.retained_fp64(q, k, heads, gated, cr.LN2).min())
    print(f"runs {runs} H={heads}: ungated min {lo_plain:.4f} density {float(plain.float().mean()):.3f}; gated min {lo_gated:.4f} density "
          f"{float(gated.float().mean()):.3f}")
    assert lo_plain < bar <= lo_gated
    # the straddling blocks and tiles are exactly the ones below the threshold; pure ones have rho = 1
    sq, sk = cr.straddling(q, ar.QB), cr.straddling(k, ar.KB)
    assert torch.equal(~(q_coh >= cr.GUARANTEE_MIN), sq.expand(heads, -1)) and torch.equal(~(k_coh >= cr.GUARANTEE_MIN), sk.expand(heads, -1))
    assert float((q_coh[:, ~sq] - 1).abs().max()) < 1e-12 and float((k_coh[:, ~sk] - 1).abs().max()) < 1e-12
    assert bool(sq.any()) or bool(sk.any())
    assert bool(gated[:, sq].all()) and bool(gated[:, :, sk].all())


# ------------------------------------------------------------------------------------------------------- the Python layer
def test_thresholds_are_checked_by_name():
    from goal_force_amd import ops
    from goal_force_amd._lib import GoalForceError
    from goal_force_amd.sparse_attention import FrameWindow, MassCover
    assert ops._block_map_min("op", "q_min", None) is None and ops._block_map_min("op", "q_min", 1) == 1.0
    assert ops._block_map_min("op", "k_min", 0.75) == 0.75
    for bad in (0, 0.0, -0.5, 1.0001, NAN, INF):
        with pytest.raises(GoalForceError, match=r"op\.q_min: expected 0 < q_min <= 1"):
            ops._block_map_min("op", "q_min", bad)
        with pytest.raises(GoalForceError, match=r"MassCover\.k_coherence: expected 0 < k_coherence <= 1"):
            MassCover(0.9, k_coherence=bad)
    with pytest.raises(GoalForceError, match=r"MassCover\.q_coherence: expected a number in \(0, 1\]"):
        MassCover(0.9, q_coherence="high")
    mc = MassCover(0.9, always=FrameWindow(1, 1), q_coherence=0.75, k_coherence=0.5)
    assert (mc.q_coherence, mc.k_coherence) == (0.75, 0.5)
    assert repr(mc) == "MassCover(0.9, always=FrameWindow(1, 1), q_coherence=0.75, k_coherence=0.5)"
    assert repr(MassCover(0.9, k_coherence=1)) == "MassCover(0.9, always=None, q_coherence=None, k_coherence=1.0)"
    assert repr(MassCover(0.9, always=FrameWindow(1, 1))) == "MassCover(0.9, always=FrameWindow(1, 1))"          # unchanged without a gate
    assert MassCover(0.9).q_coherence is None and MassCover(0.9).k_coherence is None


def test_wrappers_refuse_without_a_gpu_and_name_the_argument():
    from goal_force_amd import ops
    from goal_force_amd._lib import GoalForceError
    assert {"block_means_coherence", "block_means", "block_map_select", "block_map_from_qk"} <= set(ops.__all__)
    x = torch.zeros((256, 256), dtype=torch.bfloat16)
    with pytest.raises(GoalForceError, match=r"block_means_coherence\.x: tensor must be on the GPU"):
        ops.block_means_coherence(x, 2, 64)
    with pytest.raises(GoalForceError, match="GPU"):
        ops.block_map_from_qk(x, x, 2, 0.9, q_min=0.75, k_min=0.75)
    with pytest.raises(GoalForceError, match=r"block_map_select\.k_coherence: tensor must be on the GPU"):
        ops._block_map_coherence("block_map_select", "k_coherence", torch.ones((2, 4)), 2, 4, torch.device("cpu"))


def test_enable_sparse_attention_accepts_a_gated_pattern():
    from goal_force_amd import dit
    from goal_force_amd.sparse_attention import MassCover
    blk = dit.DiTBlock(False, 256, 2, 512)
    pattern = MassCover(0.9, q_coherence=0.75, k_coherence=0.75)
    dit.enable_sparse_attention(blk, pattern)
    assert blk.self_attn._gf_sparse is pattern
    dit.enable_sparse_attention(blk, None)


# ---------------------------------------------------------------------------------------------------- header and bindings
def test_header_declares_and_library_exports_the_gated_entry_points():
    hdr = open(os.path.join(ROOT, "include", "goalforce.h")).read()
    for sym in GATED_SYMBOLS:
        assert re.search(r"GF_API\s+[\w\s\*]+\b" + sym + r"\(", hdr), sym
    assert "1b. coherence" in hdr and "GUARANTEES" in hdr and "overflow fp32" in hdr
    from goal_force_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 20 and lib.gf_abi_version() == 20
    for sym in GATED_SYMBOLS:
        assert sym in _lib.SYMBOLS and hasattr(lib, sym), sym
    p, q, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    b = _lib.BINDINGS
    assert b["gf_block_map_gated_workspace_bytes"] == (q, [q] * 3)
    assert b["gf_block_means_coh"] == (ctypes.c_int, [p, q, p, p, q, q, q, p])
    assert b["gf_block_map_select_gated"] == (ctypes.c_int, [p] * 9 + [q] * 3 + [f] * 3 + [p])
    assert b["gf_block_map_from_qk_gated"] == (ctypes.c_int, [p, q, p, q] + [p] * 9 + [q] * 3 + [f] * 4 + [p])
    # the old entries' signatures did not move
    assert len(b["gf_block_map_from_qk"][1]) == 17 and len(b["gf_block_map_select"][1]) == 12 and len(b["gf_block_means"][1]) == 7
    # the workspace query is host arithmetic: the ungated workspace plus the two coherence arrays
    plain, gated = lib.gf_block_map_workspace_bytes(32760, 32760, 40), lib.gf_block_map_gated_workspace_bytes(32760, 32760, 40)
    assert plain + 4 * (40 * 128 + 40 * 512) <= gated <= plain + 4 * (40 * 128 + 40 * 512) + 512
    assert lib.gf_block_map_gated_workspace_bytes(256, 127, 1) == 0 and lib.gf_block_map_gated_workspace_bytes(256, 65537, 1) == 0
    # refusals that need no device: checked before any pointer is touched
    assert lib.gf_block_map_select_gated(None, None, None, None, None, None, None, None, None, 1, 4, 1, 0.9, 1.5, 0.5, None) == -1
    assert "q_min in (0, 1]" in lib.gf_last_error().decode()
    assert lib.gf_block_map_select_gated(None, None, None, None, None, None, None, None, None, 1, 4, 1, 0.9, 0.5, NAN, None) == -1
    assert "k_min in (0, 1]" in lib.gf_last_error().decode()
    assert lib.gf_block_map_from_qk_gated(None, 128, None, 128, None, None, None, None, None, None, None, None, None, 256, 127, 1, 0.1, 0.9,
                                          0.5, 0.5, None) == -1
    assert "kv_len >= 128" in lib.gf_last_error().decode()
    assert lib.gf_block_means_coh(None, 128, None, None, 64, 1, 64, None) == -1
    assert "null pointer" in lib.gf_last_error().decode()
