"""The mass-cover recipe's restatement (tests/adaptive_map_refs.py) against itself on hand-made rows, the argument checks of
sparse_attention.MassCover / ops.BlockMap.from_device, and the C ABI's declarations — everything that needs no GPU."""
import math
import os
import re

import pytest
import torch

import adaptive_map_refs as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK_MAP_SYMBOLS = ("gf_block_map_workspace_bytes", "gf_block_map_select_workspace_bytes", "gf_block_means", "gf_block_map_scores",
                     "gf_block_map_select", "gf_block_map_from_qk")
NAN, INF = float("nan"), float("inf")


def _sel(s, tau, forced=None):
    return ar.select_row(torch.tensor(s, dtype=torch.float64), tau, None if forced is None else torch.tensor(forced)).tolist()


def test_mass_one_selects_every_tile():
    assert _sel([0.0, -30.0, -5.0, 2.0], 1.0) == [True] * 4
    assert _sel([0.0, -30.0], 1.5, [False, True]) == [True] * 2


def test_smallest_top_set_that_reaches_the_mass():
    # w = 8, 4, 2, 1, 1 (W = 16): 0.5 needs {8}, then the floor adds the 4; 0.75 is reached exactly by {8, 4}; 0.8 needs the 2 as well
    s = [3.0, 2.0, 1.0, 0.0, 0.0]
    assert _sel(s, 0.5) == [True, True, False, False, False]
    assert _sel(s, 0.75) == [True, True, False, False, False]
    assert _sel(s, 0.8) == [True, True, True, False, False]
    assert _sel(s, 0.9) == [True] * 5                                   # 14 / 16 < 0.9: the tied pair comes together
    # the order of the tiles does not matter
    assert _sel([0.0, 3.0, 0.0, 1.0, 2.0], 0.8) == [False, True, False, True, True]


def test_forced_only_when_the_forced_tiles_reach_the_mass():
    s = [3.0, 2.0, 1.0, 0.0, 0.0]
    assert _sel(s, 0.5, [True, False, False, True, False]) == [True, False, False, True, False]       # F = 9 >= 8: nothing is added
    assert _sel(s, 0.75, [False, False, False, True, True]) == [True, True, False, True, True]        # F = 2: 2 + 8 + 4 = 14 >= 12
    # a forced tile's own mass counts once, whether it passes the threshold or not
    assert _sel(s, 0.6, [False, True, False, False, False]) == [True, True, False, False, False]      # F = 4: 4 + 8 >= 9.6


def test_ties_are_taken_together():
    s = [1.0, 0.0, 0.0, 0.0, 0.0, -4.0]                                    # w = 1, .5 x 4, 1/32: W = 3.03125
    assert _sel(s, 0.4) == [True, True, True, True, True, False]         # 1 < 1.2125: all four halves enter together
    assert _sel(s, 0.98) == [True, True, True, True, True, False]        # 3 / 3.03125 = 0.98969
    assert _sel(s, 0.99) == [True] * 6
    assert ar.kept_share(torch.tensor(s), torch.tensor(_sel(s, 0.4))) == pytest.approx(3 / 3.03125)
    assert _sel([0.0, 0.0, 0.0], 0.01) == [True] * 3                     # three equal tiles: no subset is a threshold set


def test_two_tile_floor_takes_the_largest_then_the_lowest_index():
    assert _sel([0.0, -20.0, -20.0, -20.0], 0.5) == [True, True, False, False]        # ties: lowest index
    assert _sel([-20.0, -20.0, 0.0, -19.0], 0.5) == [False, False, True, True]        # the largest unselected
    assert _sel([-9.0, 0.0], 0.5) == [True, True]
    # one forced tile that holds the mass alone: the floor adds the largest other
    assert _sel([0.0, -1.0, -2.0], 0.5, [True, False, False]) == [True, True, False]


def test_selection_is_monotone_in_the_mass():
    g = torch.Generator().manual_seed(5)
    taus = [0.05, 0.3, 0.5, 0.75, 0.9, 0.99, 1.0]
    for n_t in (2, 3, 17, 64):
        for _ in range(6):
            s = torch.randn(n_t, generator=g, dtype=torch.float64) * 3
            forced = torch.rand(n_t, generator=g) < 0.2
            for f in (None, forced):
                prev = None
                for tau in taus:
                    sel = ar.select_row(s, tau, f)
                    assert int(sel.sum()) >= 2 and (f is None or bool(sel[f].all()))
                    assert prev is None or bool((sel | ~prev).all()), (n_t, tau)
                    prev = sel


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_a_non_finite_score_selects_the_whole_row(bad):
    assert _sel([0.0, bad, -3.0, 5.0], 0.5) == [True] * 4
    assert _sel([bad, 0.0], 0.1, [True, False]) == [True] * 2


def test_csr_and_means_and_scores_restatement():
    mask = torch.tensor([[[True, False, True], [True, True, True]], [[False, True, True], [True, True, False]]])
    row_ptr, tile_idx = ar.csr(mask)
    assert row_ptr.tolist() == [0, 2, 5, 7, 9] and tile_idx.tolist() == [0, 2, 0, 1, 2, 1, 2, 0, 1]
    x = torch.arange(300 * 128, dtype=torch.float64).reshape(300, 128)
    m = ar.block_means(x, 1, 256)
    assert m.shape == (1, 2, 128) and torch.equal(m[0, 1], x[256:].mean(0))     # the ragged block divides by its own 44 rows
    assert ar.tile_keys(200).tolist() == [64.0, 64.0, 64.0, 8.0]
    qm, km = torch.ones((1, 1, 128), dtype=torch.float64), torch.full((1, 4, 128), 0.5, dtype=torch.float64)
    s = ar.scores(qm, km, 200, scale=math.log(2.0))
    assert ar.softmax_c(math.log(2.0)) == 1.0
    assert torch.allclose(s[0, 0], torch.tensor([70.0, 70.0, 70.0, 67.0], dtype=torch.float64))


def test_mass_cover_checks_its_arguments_by_name():
    from goal_force_amd._lib import GoalForceError
    from goal_force_amd.sparse_attention import FrameWindow, MassCover
    for bad in (0, 0.0, -0.5, 1.0001, NAN, "a lot", None):
        with pytest.raises(GoalForceError, match="0 < mass <= 1"):
            MassCover(bad)
    with pytest.raises(GoalForceError, match="static pattern"):
        MassCover(0.9, always=3)
    with pytest.raises(GoalForceError, match="data-dependent"):
        MassCover(0.9, always=MassCover(0.5))
    mc = MassCover(0.9, always=FrameWindow(1, 1), keep_last=True)
    assert repr(mc) == "MassCover(0.9, always=FrameWindow(1, 1))" and mc.keep_last and mc.last_map is None
    assert repr(MassCover(1)) == "MassCover(1.0, always=None)"
    with pytest.raises(GoalForceError, match="no map without q and k"):
        mc((3, 20, 35))


def test_enable_sparse_attention_accepts_either_kind_of_pattern():
    from goal_force_amd import dit
    from goal_force_amd._lib import GoalForceError
    from goal_force_amd.sparse_attention import FrameWindow, MassCover
    blk = dit.DiTBlock(False, 256, 2, 512)
    for pattern in (MassCover(0.9), FrameWindow(1, 1), None):
        dit.enable_sparse_attention(blk, pattern)
        assert blk.self_attn._gf_sparse is pattern
    with pytest.raises(GoalForceError, match="expected a callable"):
        dit.enable_sparse_attention(blk, 0.9)


def test_from_device_checks_its_arguments_by_name():
    from goal_force_amd import ops
    from goal_force_amd._lib import GoalForceError
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)      # noqa: E731
    bm = ops.BlockMap.from_device(i32(0, 2, 5), i32(0, 1, 0, 1, 2, 9, 9), i32(0, 1), 2, 1, 3)
    assert (bm.n_maps, bm.n_qblocks, bm.n_tiles) == (2, 1, 3) and bm.q_len == (1, 256) and bm.kv_len == (129, 192)
    assert "_density" not in bm.__dict__                                             # nothing was read
    assert bm.counts().tolist() == [[2], [3]]
    assert bm.mask().tolist() == [[[True, True, False]], [[True, True, True]]]       # the buffer's unused tail is ignored
    assert bm.density == pytest.approx(5 / 6)
    host = ops.BlockMap(bm.mask(), head_map=[0, 1])
    assert host.density == bm.density and torch.equal(host.row_ptr, bm.row_ptr) and torch.equal(host.tile_idx, bm.tile_idx[:5])
    with pytest.raises(GoalForceError, match=r"row_ptr: expected \[3\]"):
        ops.BlockMap.from_device(i32(0, 2), i32(0, 1, 0, 1), None, 2, 1, 3)
    with pytest.raises(GoalForceError, match="tile_idx: expected room"):
        ops.BlockMap.from_device(i32(0, 2, 5), i32(0, 1, 2), None, 2, 1, 3)
    with pytest.raises(GoalForceError, match="row_ptr: expected a contiguous 1-D int32"):
        ops.BlockMap.from_device(torch.tensor([0, 2, 5]), i32(0, 1, 0, 1), None, 2, 1, 3)
    with pytest.raises(GoalForceError, match="n_tiles >= 2"):
        ops.BlockMap.from_device(i32(0, 2), i32(0, 0), None, 1, 1, 1)
    with pytest.raises(GoalForceError, match="expected integer"):
        ops.BlockMap.from_device(i32(0, 2), i32(0, 1), None, 1, "one", 2)


def test_forced_bits_of_an_always_map():
    from goal_force_amd import ops
    from goal_force_amd._lib import GoalForceError
    mask = torch.zeros((2, 70), dtype=torch.bool)
    mask[0, [0, 31, 32, 69]] = True
    mask[1, [5, 63, 64]] = True
    bm = ops.BlockMap(mask)
    bits = bm.forced_bits("cpu")
    assert bits.dtype == torch.int32 and bits.shape == (2, 3)
    assert [[int(w) & 0xFFFFFFFF for w in row] for row in bits.tolist()] == [[0x80000001, 0x1, 0x20], [0x20, 0x80000000, 0x1]]
    assert bm.forced_bits("cpu") is bits                                             # built once
    with pytest.raises(GoalForceError, match="one map for all heads"):
        ops.BlockMap(torch.ones((2, 2, 4), dtype=torch.bool)).forced_bits("cpu")


def test_wrappers_refuse_without_a_gpu_and_bad_shapes_by_name():
    from goal_force_amd import ops
    from goal_force_amd._lib import GoalForceError
    q = torch.zeros((256, 256), dtype=torch.bfloat16)
    with pytest.raises(GoalForceError, match="GPU"):
        ops.block_map_from_qk(q, q, 2, 0.9)
    with pytest.raises(GoalForceError, match="GPU"):
        ops.block_means(q, 2, 64)
    with pytest.raises(GoalForceError, match="GPU"):
        ops.block_map_select(torch.zeros((2, 1, 4)), 0.9)
    with pytest.raises(GoalForceError, match="at least 128 keys"):
        ops._block_map_shape("block_map_from_qk", 256, 127)
    with pytest.raises(GoalForceError, match="at most 1024 key tiles"):
        ops._block_map_shape("block_map_from_qk", 256, 65537)
    assert ops._block_map_shape("block_map_from_qk", 2100, 2100) == (9, 33)
    with pytest.raises(GoalForceError, match="0 < mass <= 1"):
        ops._block_map_mass("block_map_from_qk", 1.5)


def test_header_declares_and_library_exports_the_block_map_entry_points():
    hdr = open(os.path.join(ROOT, "include", "goalforce.h")).read()
    for s in BLOCK_MAP_SYMBOLS:
        assert re.search(r"GF_API\s+[\w\s\*]+\b" + s + r"\(", hdr), s
    from goal_force_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 20 and lib.gf_abi_version() == 20
    for s in BLOCK_MAP_SYMBOLS:
        assert s in _lib.SYMBOLS and hasattr(lib, s), s
    import ctypes
    assert _lib.BINDINGS["gf_block_map_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int64] * 3)
    assert len(_lib.BINDINGS["gf_block_map_from_qk"][1]) == 17 and _lib.BINDINGS["gf_block_map_from_qk"][1][-3:-1] == [ctypes.c_float] * 2
    # the workspace queries are host arithmetic: no device needed.  Production: 40 heads, 32760 tokens = 128 blocks x 512 tiles
    n = lib.gf_block_map_workspace_bytes(32760, 32760, 40)
    assert n >= 4 * (40 * 128 * 128 + 40 * 512 * 128 + 40 * 128 * 512) + 4 * 5120 * 17 and n < 32 * 2 ** 20
    assert lib.gf_block_map_select_workspace_bytes(128, 512, 40) >= 4 * 5120 * 17
    assert lib.gf_block_map_workspace_bytes(256, 127, 1) == 0 and lib.gf_block_map_workspace_bytes(256, 65537, 1) == 0
    # the entries refuse these shapes by name before touching any pointer
    assert lib.gf_block_map_from_qk(None, 128, None, 128, None, None, None, None, None, None, None, 256, 127, 1, 0.1, 0.9, None) == -1
    assert "kv_len >= 128" in lib.gf_last_error().decode()
    assert lib.gf_block_map_from_qk(None, 128, None, 128, None, None, None, None, None, None, None, 256, 65537, 1, 0.1, 0.9, None) == -1
    assert "at most 1024 key tiles" in lib.gf_last_error().decode()
    assert lib.gf_block_map_select(None, None, None, None, None, None, None, 1, 1025, 1, 0.9, None) == -1
    assert "2 .. 1024 key tiles" in lib.gf_last_error().decode()
