"""Block-sparse self-attention without a GPU: the FrameWindow pattern against a token-level restatement of its definition, its
figures at the production grid, ops.BlockMap (CSR round trip, validation), dit.enable_sparse_attention (which blocks it
switches) and the refusals of a switched block, each raised before any kernel wrapper is reached."""
import pytest
import torch

import gen_inputs as gi
import sparse_refs as sr

BF = torch.bfloat16


@pytest.mark.parametrize("grid,window,sink", [((5, 6, 16), 1, 1), ((7, 4, 20), 1, 1), ((9, 5, 13), 1, 1), ((9, 5, 13), 2, 0)])
def test_frame_window_is_its_token_level_definition(grid, window, sink):
    """Ragged last query block and last tile (S = 480 / 560 / 585), frames that straddle tiles, with and without the sink."""
    from goal_force_amd.sparse_attention import FrameWindow
    fw = FrameWindow(window, sink)
    want = sr.frame_window_by_tokens(grid, window, sink)
    assert torch.equal(fw.mask(grid), want)
    bm = fw(grid)
    assert (bm.n_maps, bm.n_qblocks, bm.n_tiles) == (1,) + tuple(want.shape) and torch.equal(bm.mask()[0], want)
    assert fw(grid) is bm, "memoised per grid"
    assert bool(want.any()) and not bool(want.all()), "the case must select some pairs and leave some out"


def test_frame_window_at_the_production_grid():
    """832 x 480 x 81 frames: grid (21, 30, 52), S = 32760 -> 128 query blocks x 512 tiles.  The figures the documents quote."""
    from goal_force_amd.sparse_attention import FrameWindow
    grid = (21, 30, 52)
    dens, counts = {}, {}
    for w in (1, 2, 3, 5):
        bm = FrameWindow(w, 1)(grid)
        assert (bm.n_maps, bm.n_qblocks, bm.n_tiles) == (1, 128, 512)
        assert bm.q_len[0] <= 32760 <= bm.q_len[1] and bm.kv_len[0] <= 32760 <= bm.kv_len[1]
        dens[w], counts[w] = round(bm.density, 3), bm.counts()[0]
    assert dens == {1: 0.190, 2: 0.274, 3: 0.352, 5: 0.496}
    assert (int(counts[3].min()), int(counts[3].max())) == (98, 221) and (int(counts[1].min()), int(counts[1].max())) == (49, 124)
    for w in (1, 3):
        assert set((counts[w] % 2).tolist()) == {0, 1}, "rows of even and of odd length: both tails of the kernel's phase loop"
    assert bool(FrameWindow(20, 1).mask(grid).all()) and bool(FrameWindow(25, 0).mask(grid).all())
    assert not bool(FrameWindow(19, 0).mask(grid).all())


def test_block_map_csr_round_trip_and_validation():
    from goal_force_amd import ops
    from goal_force_amd._lib import GoalForceError
    g = torch.Generator().manual_seed(3)
    mask = torch.rand((2, 5, 9), generator=g) < 0.4
    mask[:, :, 0] = True
    mask[:, :, 7] = True                                     # at least 2 per row
    bm = ops.BlockMap(mask, head_map=[0, 1, 1, 0])
    assert (bm.n_maps, bm.n_qblocks, bm.n_tiles) == (2, 5, 9) and torch.equal(bm.mask(), mask)
    assert bm.row_ptr.dtype == bm.tile_idx.dtype == bm.head_map.dtype == torch.int32
    assert bm.row_ptr.tolist()[0] == 0 and bm.row_ptr.tolist()[-1] == int(mask.sum()) == bm.tile_idx.numel()
    rp, ti = bm.row_ptr.tolist(), bm.tile_idx.tolist()
    for r in range(10):
        row = ti[rp[r]:rp[r + 1]]
        assert row == sorted(row) and row == mask.reshape(10, 9)[r].nonzero().flatten().tolist()
    assert bm.q_len == (1025, 1280) and bm.kv_len == (513, 576)
    assert abs(bm.density - float(mask.double().mean())) < 1e-12 and torch.equal(bm.counts(), mask.sum(2))
    assert bm.to("cpu") is bm
    one = ops.BlockMap(mask[0])                              # a 2-D array is one map
    assert one.n_maps == 1 and one.head_map is None and torch.equal(one.mask()[0], mask[0])
    starved = mask.clone()
    starved[1, 3] = False
    starved[1, 3, 4] = True
    with pytest.raises(GoalForceError, match=r"at least 2 tiles in every row, got 1 in map 1, query block 3"):
        ops.BlockMap(starved)
    with pytest.raises(GoalForceError, match=r"expected \[n_maps, n_qblocks, n_tiles\]"):
        ops.BlockMap(torch.ones((2, 2, 2, 2), dtype=torch.bool))
    with pytest.raises(GoalForceError, match="expected a CPU bool array"):
        ops.BlockMap(torch.ones((2, 2, 4)))
    with pytest.raises(GoalForceError, match=r"head_map: expected map numbers in \[0, 2\)"):
        ops.BlockMap(mask, head_map=[0, 2])
    with pytest.raises(GoalForceError, match=r"head_map: expected map numbers in \[0, 2\)"):
        ops.BlockMap(mask, head_map=[-1, 0])


def test_flash_attn_sparse_checks_its_operands_before_the_library():
    from goal_force_amd import ops
    from goal_force_amd._lib import GoalForceError
    with pytest.raises(GoalForceError, match="must be on the GPU"):
        ops.flash_attn_sparse(torch.zeros((256, 128), dtype=BF), torch.zeros((256, 128), dtype=BF), torch.zeros((256, 128), dtype=BF), 1,
                              ops.BlockMap(torch.ones((1, 4), dtype=torch.bool)))


def _models():
    from goal_force_amd.controlnet import ControlNet
    from goal_force_amd.dit import WanModel
    cfg = dict(gi.TINY, num_layers=3)
    return (WanModel(has_image_input=False, require_clip_embedding=False, **cfg),
            ControlNet(2, dim=cfg["dim"], num_heads=cfg["num_heads"], ffn_dim=cfg["ffn_dim"]))


def test_enable_sparse_attention_switches_the_blocks_it_is_told_to():
    from goal_force_amd import dit
    from goal_force_amd._lib import GoalForceError
    from goal_force_amd.sparse_attention import FrameWindow
    model, cn = _models()
    fw = FrameWindow(1, 1)

    def state(m):
        return [getattr(b.self_attn, "_gf_sparse", None) for b in m.modules() if isinstance(b, dit.DiTBlock)]

    assert state(model) == [None] * 3 and state(cn) == [None] * 2
    assert dit.enable_sparse_attention(model, fw) is model and state(model) == [fw] * 3
    dit.enable_sparse_attention(model, fw, dense_blocks=2)
    assert state(model) == [None, None, fw]
    dit.enable_sparse_attention(cn, fw, dense_blocks=1)
    assert state(cn) == [None, fw]
    both = torch.nn.ModuleDict({"dit": model, "controlnet": cn})                 # what a pipeline is to .modules(): both stacks
    dit.enable_sparse_attention(both, fw, dense_blocks=1)
    assert state(model) == [None, fw, fw] and state(cn) == [None, fw], "dense_blocks counts inside every stack"
    dit.enable_sparse_attention(both, None)
    assert state(model) == [None] * 3 and state(cn) == [None] * 2

    def per_head(grid):
        raise AssertionError("not called by the switch")
    dit.enable_sparse_attention(model.blocks[1], per_head)                          # a block on its own; any callable
    assert state(model) == [None, per_head, None]
    with pytest.raises(GoalForceError, match="expected a callable"):
        dit.enable_sparse_attention(model, "window")
    with pytest.raises(GoalForceError, match="dense_blocks"):
        dit.enable_sparse_attention(model, fw, dense_blocks=-1)


def test_pipeline_has_the_dense_steps_attribute_and_takes_the_switch():
    from goal_force_amd import dit
    from goal_force_amd.pipeline import WanVideoPipeline
    from goal_force_amd.sparse_attention import FrameWindow
    model, cn = _models()
    pipe = WanVideoPipeline.from_modules(model, None, cn, None, device="cpu")
    assert pipe.sparse_dense_steps == 0
    fw = FrameWindow(2, 1)
    dit.enable_sparse_attention(pipe, fw, dense_blocks=1)
    assert [b.self_attn._gf_sparse for b in model.blocks] == [None, fw, fw]
    assert [b.self_attn._gf_sparse for b in cn.controlnet_dit.blocks] == [None, fw]


def test_a_switched_block_refuses_by_name_before_any_kernel(monkeypatch):
    """Training (`keep`), the sage backend, sequence parallelism, fewer tokens than VT_MIN_KV and rotary phases without a grid: a
    GoalForceError that names the reason, raised before the first projection (dit.linear and the ops wrappers are booby-trapped);
    under pipe.sparse_dense_steps (attend(dense=True)) the same block goes down the dense path instead.  training.DiTBlockFn refuses a
    switched block at every keep level: with level "none" it calls attend with keep=None, and its backward differentiates the
    dense attention."""
    from goal_force_amd import dit, ops, training
    from goal_force_amd._lib import GoalForceError
    from goal_force_amd.sparse_attention import FrameWindow

    def trap(*a, **k):
        raise AssertionError("a kernel wrapper was reached")
    for name in ("flash_attn", "flash_attn_sparse", "sage_attn", "rmsnorm_rope", "linear_vt32", "gemm"):
        monkeypatch.setattr(ops, name, trap)
    monkeypatch.setattr(dit, "linear", trap)
    blk = dit.DiTBlock(False, 256, 2, 512).to(BF)
    sa = blk.self_attn
    freqs3 = dit.precompute_freqs_cis_3d(128)
    big, small = (6, 16, 24), (3, 4, 6)
    rope_big = dit.RopeTable.from_grid(freqs3, *big, "cpu")
    assert rope_big.grid == big and rope_big.tokens == 2304
    x_big, x_small = torch.zeros((2304, 256), dtype=BF), torch.zeros((72, 256), dtype=BF)
    dit.enable_sparse_attention(blk, FrameWindow(1, 1))
    with pytest.raises(GoalForceError, match="no sparse backward"):
        sa.attend(x_big, rope_big, keep={})
    with pytest.raises(GoalForceError, match="sequence parallelism"):
        sa.attend(x_big, rope_big, sp=object())
    with pytest.raises(GoalForceError, match=r"at least 2048 tokens .* got 72"):
        sa.attend(x_small, dit.RopeTable.from_grid(freqs3, *small, "cpu"))
    with pytest.raises(GoalForceError, match="needs the token grid"):
        sa.attend(x_big, dit._as_rope(sr.rope_complex(freqs3, *big)[:, None, :], "cpu"))
    with pytest.raises(GoalForceError, match="expected 2304 tokens for the grid"):
        sa.attend(x_small, rope_big)
    dit.enable_sage_attention(blk)
    with pytest.raises(GoalForceError, match="enable_sage_attention"):
        sa.attend(x_big, rope_big)
    dit.enable_sage_attention(blk, False)
    dit.enable_sparse_attention(blk, lambda grid: "not a map")
    with pytest.raises(GoalForceError, match="expected the pattern to return an ops.BlockMap"):
        sa.attend(x_big, rope_big)
    # a dense step: the switch is not consulted, the block goes on to its first projection
    dit.enable_sparse_attention(blk, FrameWindow(1, 1))
    with pytest.raises(AssertionError, match="a kernel wrapper was reached"):
        sa.attend(x_big, rope_big, keep={}, dense=True)
    ctx2, t_mod = torch.zeros((7, 256), dtype=BF), torch.zeros((1, 6, 256), dtype=BF)
    for level in ("none", "attn"):
        old = training.set_keep_level(level)
        try:
            with pytest.raises(GoalForceError, match="enable_sparse_attention is refused"):
                training.DiTBlockFn.apply(blk, rope_big, x_big, ctx2, t_mod, *training._block_params(blk))
        finally:
            training.set_keep_level(old)
    dit.enable_sparse_attention(blk, None)
    with pytest.raises(AssertionError, match="a kernel wrapper was reached"):
        sa.attend(x_small, rope_big)
