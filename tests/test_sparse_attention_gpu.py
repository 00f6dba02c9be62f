"""Block-sparse self-attention on the GPU (gf_flash_attn_fwd_vt32_sparse, ops.flash_attn_sparse, dit.enable_sparse_attention,
pipe.sparse_dense_steps).  The exact bar: a query block's 256 rows computed over its selected tiles are BIT-identical — output and
log-sum-exp — to the dense kernel 3 (gf_flash_attn_fwd_vt32) run on those tiles' K / V rows gathered in order: the same arithmetic
in the same order.  The reference has no sparse branch, so there is no golden; fp64 restatements give the accuracy bars."""
import math
import types

import pytest
import torch

import gen_inputs as gi
import sparse_refs as sr

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SQ, SKV, NT = 600, 2085, 33          # three query blocks (the last one ragged), 33 key tiles (the last one ragged: 37 keys)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _row(g, count, tile0, last):
    """`count` ascending tiles of 0 .. NT-1, seeded; with / without tile 0, with / without the ragged last tile."""
    if count == NT:
        return list(range(NT))
    fixed = ([0] if tile0 else []) + ([NT - 1] if last else [])
    inner = (torch.randperm(NT - 2, generator=g)[: count - len(fixed)] + 1).tolist()
    return sorted(fixed + inner)


def _maps():
    """Three seeded maps of three rows each: the row lengths 2, 3, 4, 5, 6, 7 and 33 reach every branch of the kernel's prologue /
    steady-pair / odd-phase / last-phase structure; rows with and without tile 0 (the first selected tile sets the running
    maximum, whatever its number) and with and without the ragged last tile."""
    g = torch.Generator().manual_seed(20)
    spec = [[(2, False, False), (3, True, True), (NT, True, True)],
            [(4, False, False), (5, True, True), (6, False, True)],
            [(7, True, False), (2, True, False), (3, False, True)]]
    masks = []
    for rows in spec:
        m = torch.zeros((3, NT), dtype=torch.bool)
        for b, (count, tile0, last) in enumerate(rows):
            m[b, _row(g, count, tile0, last)] = True
        assert m.sum(1).tolist() == [r[0] for r in rows]
        masks.append(m)
    return masks


@pytest.fixture(scope="module")
def data():
    """Operands for 3 heads and for 8 heads (8: the XCD-aware head / query-block mapping), uploaded once; the fp64 references of
    the three maps at 3 heads."""
    out = types.SimpleNamespace(masks=_maps(), ops=None, t={})
    from goal_force_amd import ops
    out.ops = ops
    for heads in (3, 8):
        g = torch.Generator().manual_seed(100 + heads)
        q, k, v = (torch.randn((n, heads * 128), generator=g).to(BF) for n in (SQ, SKV, SKV))
        out.t[heads] = types.SimpleNamespace(q=q, k=k, v=v, dq=q.cuda(), dk=k.cuda(), dv=v.cuda())
    return out


def _assert_blocks_equal_gathered_dense(ops, q, k, v, heads, mask, got, got_lse, scale=None, head_cols=None):
    """Every query block of `got` / `got_lse` against the dense kernel 3 on its gathered keys.  head_cols: compare one head only
    (its columns of q / k / v / got, a one-head dense call)."""
    cols = slice(None) if head_cols is None else slice(128 * head_cols, 128 * head_cols + 128)
    nh = heads if head_cols is None else 1
    for b in range(mask.shape[0]):
        tiles = mask[b].nonzero().flatten().tolist()
        rows = slice(256 * b, min(256 * b + 256, q.shape[0]))
        kg, vg = sr.gather_rows(k[:, cols], tiles, k.shape[0]), sr.gather_rows(v[:, cols], tiles, k.shape[0])
        assert kg.shape[0] >= 128, "the dense entry's own contract"
        want, want_lse = sr.dense_kernel3(ops, q[rows, cols], kg, vg, nh, scale)
        torch.cuda.synchronize()
        assert torch.equal(got[rows, cols].view(torch.int16), want.view(torch.int16)), f"query block {b} (tiles {tiles}): output bits"
        lse_cols = slice(None) if head_cols is None else slice(head_cols, head_cols + 1)
        assert torch.equal(got_lse[rows, lse_cols].view(torch.int32), want_lse.view(torch.int32)), f"query block {b} (tiles {tiles}): lse bits"


@pytest.mark.parametrize("heads", [3, 8])
def test_full_map_is_the_dense_kernel_bit_for_bit(data, heads):
    ops, t = data.ops, data.t[heads]
    bm = ops.BlockMap(torch.ones((3, NT), dtype=torch.bool), device="cuda")
    assert bm.density == 1.0
    got, lse = ops.flash_attn_sparse(t.dq, t.dk, t.dv, heads, bm, lse=True)
    want, want_lse = sr.dense_kernel3(ops, t.dq, t.dk, t.dv, heads)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and torch.equal(lse.view(torch.int32), want_lse.view(torch.int32))
    plain = ops.flash_attn_sparse(t.dq, t.dk, t.dv, heads, bm)                  # without the lse output: the same bits
    assert torch.equal(plain, got)


@pytest.mark.parametrize("heads", [3, 8])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_random_maps_equal_the_dense_kernel_on_gathered_keys(data, heads, which):
    """Bit identity per query block; the whole output within rel-L2 4e-3 of the fp64 masked softmax (test_flash_attn_kernel3_vs_fp64's
    bar).  The lse (log2 domain) is held to what the number formats allow: the kernel rounds Q c (c = log2 e / sqrt 128) to bf16, so a
    score moves by at most 2^-9 c |q| |k|, the lse by no more than the largest such move, plus 2^-8 for the bf16 probabilities it sums."""
    ops, t, mask = data.ops, data.t[heads], data.masks[which]
    bm = ops.BlockMap(mask, device="cuda")
    got, lse = ops.flash_attn_sparse(t.dq, t.dk, t.dv, heads, bm, lse=True)
    _assert_blocks_equal_gathered_dense(ops, t.dq, t.dk, t.dv, heads, mask, got, lse)
    ref, ref_lse = sr.masked_attention_fp64(t.q, t.k, t.v, heads, mask)
    e, e_lse = rel_l2(got.cpu(), ref), float((lse.cpu().double() - ref_lse).abs().max())
    print(f"map {which}, {heads} heads (rows of {mask.sum(1).tolist()} tiles): rel-L2 vs fp64 masked softmax {e:.3e}, lse max abs {e_lse:.3e}")
    assert e < 4e-3 and bool(torch.isfinite(got.float()).all())
    c = math.log2(math.e) / math.sqrt(128)
    qn, kn = (float(x.float().reshape(x.shape[0], heads, 128).norm(dim=-1).max()) for x in (t.q, t.k))
    assert e_lse <= 2.0 ** -9 * c * qn * kn + 2.0 ** -8


@pytest.mark.parametrize("heads", [3, 8])
def test_peaky_logits_rescale_after_a_skipped_prefix(data, heads):
    """q x 8 (logit std 8): later tiles raise the running maximum past the lazy-rescale threshold, so O is rescaled against the maximum
    the FIRST SELECTED tile set — "first" keyed on tile 0 instead of list position 0 fails the rows without tile 0 here."""
    ops, t = data.ops, data.t[heads]
    q8 = (t.q.float() * 8).to(BF).cuda()
    for mask in data.masks:
        got, lse = ops.flash_attn_sparse(q8, t.dk, t.dv, heads, ops.BlockMap(mask, device="cuda"), lse=True)
        _assert_blocks_equal_gathered_dense(ops, q8, t.dk, t.dv, heads, mask, got, lse)
        assert bool(torch.isfinite(got.float()).all()) and bool(torch.isfinite(lse).all())


def test_head_map_gives_every_head_its_own_map(data):
    ops, t = data.ops, data.t[8]
    masks = torch.stack([data.masks[1], data.masks[2]])
    head_map = [h % 2 for h in range(8)]
    bm = ops.BlockMap(masks, head_map=head_map, device="cuda")
    got, lse = ops.flash_attn_sparse(t.dq, t.dk, t.dv, 8, bm, lse=True)
    for h in range(8):
        _assert_blocks_equal_gathered_dense(ops, t.dq, t.dk, t.dv, 8, masks[head_map[h]], got, lse, head_cols=h)
    ref, _ = sr.masked_attention_fp64(t.q, t.k, t.v, 8, masks, head_map=head_map)
    assert rel_l2(got.cpu(), ref) < 4e-3


def test_strided_operands_and_out(data):
    """q, k and v as column slices of fused buffers, `out` a column slice of a wider one: the same bits as on contiguous operands, and
    nothing written outside the slice; a caller's scale."""
    ops, t, mask = data.ops, data.t[3], data.masks[1]
    bm = ops.BlockMap(mask, device="cuda")
    W = 3 * 128
    qbuf = torch.cat([torch.full((SQ, W), 3.0, dtype=BF, device="cuda"), t.dq], dim=1)
    kvbuf = torch.cat([t.dk, t.dv], dim=1)
    obuf = torch.full((SQ, 2 * W), 7.0, dtype=BF, device="cuda")
    want = ops.flash_attn_sparse(t.dq, t.dk, t.dv, 3, bm, scale=0.07)
    got = ops.flash_attn_sparse(qbuf[:, W:], kvbuf[:, :W], kvbuf[:, W:], 3, bm, out=obuf[:, W:], scale=0.07)
    assert got.data_ptr() == obuf[:, W:].data_ptr() and torch.equal(got, want)
    assert bool((obuf[:, :W] == 7.0).all())
    lse = ops.flash_attn_sparse(t.dq, t.dk, t.dv, 3, bm, scale=0.07, lse=True)[1]
    _assert_blocks_equal_gathered_dense(ops, t.dq, t.dk, t.dv, 3, mask, want, lse, scale=0.07)


def test_wrapper_refuses_a_map_of_another_shape(data):
    from goal_force_amd._lib import GoalForceError
    ops, t = data.ops, data.t[3]
    with pytest.raises(GoalForceError, match=r"expected \[3 query blocks, 33 tiles\]"):
        ops.flash_attn_sparse(t.dq, t.dk, t.dv, 3, ops.BlockMap(torch.ones((3, 32), dtype=torch.bool), device="cuda"))
    with pytest.raises(GoalForceError, match="expected the map on cuda"):
        ops.flash_attn_sparse(t.dq, t.dk, t.dv, 3, ops.BlockMap(torch.ones((3, NT), dtype=torch.bool)))
    with pytest.raises(GoalForceError, match=r"expected a head_map of \[3\]"):
        ops.flash_attn_sparse(t.dq, t.dk, t.dv, 3, ops.BlockMap(torch.ones((1, 3, NT), dtype=torch.bool), head_map=[0, 0], device="cuda"))
    with pytest.raises(GoalForceError, match="128 keys"):
        ops.flash_attn_sparse(t.dq, t.dk[:100], t.dv[:100], 3, ops.BlockMap(torch.ones((3, 2), dtype=torch.bool), device="cuda"))


# ------------------------------------------------------------------ the module
GRID = (6, 16, 24)               # 21 frames of 256 x 384: S = 2304 tokens = 9 query blocks x 36 tiles, six tiles per frame
S = GRID[0] * GRID[1] * GRID[2]


@pytest.fixture(scope="module")
def block():
    from goal_force_amd import dit
    g = torch.Generator().manual_seed(7)
    blk = dit.DiTBlock(False, 256, 2, 512).to(BF)
    for name, p_ in blk.named_parameters():
        p_.data.copy_((torch.randn(p_.shape, generator=g) * (0.06 if p_.dim() == 2 else 0.02)).to(BF))
    for n in (blk.self_attn.norm_q, blk.self_attn.norm_k, blk.cross_attn.norm_q, blk.cross_attn.norm_k):
        n.weight.data.fill_(1.0)
    blk = blk.cuda()
    freqs3 = dit.precompute_freqs_cis_3d(128)
    x, ctx, t_mod = gi.block_inputs(256, S, gi.TINY_CTX_LEN, seed=31)
    return types.SimpleNamespace(blk=blk, rope=dit.RopeTable.from_grid(freqs3, *GRID, "cuda"), freqs=sr.rope_complex(freqs3, *GRID),
                                 x=x, dx=x.cuda(), ctx=ctx.cuda(), t_mod=t_mod.cuda())


def _spy(monkeypatch, ops, names):
    """Count the calls of ops wrappers (the real ones still run)."""
    calls = []
    for name in names:
        real = getattr(ops, name)

        def wrapped(*a, _real=real, _name=name, **k):
            calls.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)
    return calls


def test_block_with_an_all_selecting_pattern_is_the_dense_block(block, monkeypatch):
    """FrameWindow(10) at 6 frames selects every tile: the switched block computes the dense block's bits, through
    ops.flash_attn_sparse; pattern=None gives back the dense path (no sparse call, the bits from before)."""
    from goal_force_amd import dit, ops
    from goal_force_amd.sparse_attention import FrameWindow
    b = block
    before = b.blk(b.dx, b.ctx, b.t_mod, b.rope).clone()
    calls = _spy(monkeypatch, ops, ["flash_attn_sparse"])
    try:
        dit.enable_sparse_attention(b.blk, FrameWindow(10))
        assert FrameWindow(10)(GRID).density == 1.0
        on = b.blk(b.dx, b.ctx, b.t_mod, b.rope).clone()
        assert calls == ["flash_attn_sparse"] and torch.equal(on, before)
    finally:
        dit.enable_sparse_attention(b.blk, None)
    del calls[:]
    after = b.blk(b.dx, b.ctx, b.t_mod, b.rope)
    assert not calls and torch.equal(after, before)


def test_self_attention_under_a_frame_window_is_as_accurate_as_the_dense_module(block):
    """SelfAttention.forward with FrameWindow(1, 1) against the fp64 restatement of the MASKED module; the bar is the dense module's
    own error against the unmasked fp64 restatement, measured here on the same weights and input, x 1.25 (test_kernels_gpu.py's
    margin for "no coarser than the yardstick") — no absolute number fixed ahead of time."""
    from goal_force_amd import dit
    from goal_force_amd.sparse_attention import FrameWindow
    b, sa = block, block.blk.self_attn
    sd = {k: v.detach().cpu() for k, v in sa.state_dict().items()}
    fw = FrameWindow(1, 1)
    mask = fw.mask(GRID)
    assert 0.3 < float(mask.float().mean()) < 0.8
    dense = sa(b.dx, b.rope).float().cpu()[0]
    try:
        dit.enable_sparse_attention(b.blk, fw)
        sparse = sa(b.dx, b.rope).float().cpu()[0]
    finally:
        dit.enable_sparse_attention(b.blk, None)
    ref_dense = sr.self_attention_fp64(b.x[0], b.freqs, sd, 2, sa.norm_q.eps)
    ref_sparse = sr.self_attention_fp64(b.x[0], b.freqs, sd, 2, sa.norm_q.eps, block_mask=mask)
    e_dense, e_sparse, apart = rel_l2(dense, ref_dense), rel_l2(sparse, ref_sparse), rel_l2(ref_sparse, ref_dense)
    print(f"SelfAttention S={S}: dense vs fp64 {e_dense:.3e}; FrameWindow(1,1) (density {float(mask.float().mean()):.3f}) vs masked fp64 "
          f"{e_sparse:.3e}; masked vs unmasked fp64 {apart:.3e}")
    assert apart > 10 * e_dense, "the mask must matter at this input, or the comparison shows nothing"
    assert e_sparse <= 1.25 * e_dense


def test_fp8_linears_write_the_sparse_kernels_vt_operand(monkeypatch):
    """Config 5 (enable_fp8) on a block wide enough for the V^T-by-GEMM route (dim 512): the switched block calls
    ops.linear_vt32_fp8 and hands its V^T to ops.flash_attn_sparse; with bf16 linears it is ops.linear_vt32.  An all-selecting
    pattern: the bits of the dense block on either route."""
    from goal_force_amd import dit, ops
    from goal_force_amd.sparse_attention import FrameWindow
    g = torch.Generator().manual_seed(9)
    blk = dit.DiTBlock(False, 512, 4, 512).to(BF)
    for p_ in blk.parameters():
        p_.data.copy_((torch.randn(p_.shape, generator=g) * (0.04 if p_.dim() == 2 else 0.02)).to(BF))
    blk = blk.cuda()
    rope = dit.RopeTable.from_grid(dit.precompute_freqs_cis_3d(128), *GRID, "cuda")
    x, ctx, t_mod = (t.cuda() for t in gi.block_inputs(512, S, gi.TINY_CTX_LEN, seed=32))
    for fp8, route in ((False, "linear_vt32"), (True, "linear_vt32_fp8")):
        dit.enable_fp8(blk, fp8)
        dense = blk(x, ctx, t_mod, rope).clone()
        dit.enable_sparse_attention(blk, FrameWindow(10))
        with monkeypatch.context() as mp:
            calls = _spy(mp, ops, ["linear_vt32", "linear_vt32_fp8", "flash_attn_sparse", "flash_attn"])
            on = blk(x, ctx, t_mod, rope)
        dit.enable_sparse_attention(blk, None)
        assert route in calls and "flash_attn_sparse" in calls and calls.count("linear_vt32") + calls.count("linear_vt32_fp8") == 1, calls
        assert torch.equal(on, dense), route


def test_switched_block_refuses_on_the_device(block):
    from goal_force_amd import dit
    from goal_force_amd._lib import GoalForceError
    from goal_force_amd.sparse_attention import FrameWindow
    b, sa = block, block.blk.self_attn
    try:
        dit.enable_sparse_attention(b.blk, FrameWindow(1, 1))
        with pytest.raises(GoalForceError, match="no sparse backward"):
            sa.attend(b.dx[0], b.rope, keep={})
        with pytest.raises(GoalForceError, match="sequence parallelism"):
            sa.attend(b.dx[0], b.rope, sp=types.SimpleNamespace(size=2, rank=0))
        with pytest.raises(GoalForceError, match="needs the token grid"):
            sa(b.dx, b.freqs[:, None, :])                                           # a caller's complex freqs
        small = dit.RopeTable.from_grid(dit.precompute_freqs_cis_3d(128), 3, 4, 6, "cuda")
        with pytest.raises(GoalForceError, match="at least 2048 tokens"):
            sa.attend(b.dx[0, :72].contiguous(), small)
        dit.enable_sage_attention(b.blk)
        with pytest.raises(GoalForceError, match="enable_sage_attention"):
            sa.attend(b.dx[0], b.rope)
    finally:
        dit.enable_sage_attention(b.blk, False)
        dit.enable_sparse_attention(b.blk, None)


# ------------------------------------------------------------------ the pipeline
@pytest.fixture(scope="module")
def pipe_setup():
    """Two tiny experts (2 blocks each) and their ControlNets (1 block) as in test_teacache_gpu.py, at 21 frames of 256 x 384."""
    from goal_force_amd.controlnet import ControlNet
    from goal_force_amd.dit import WanModel
    from goal_force_amd.pipeline import WanVideoPipeline
    cfg = gi.TINY

    def expert(seed):
        m = WanModel(has_image_input=False, require_clip_embedding=False, **cfg)
        m.load_state_dict(gi.dit_sd(cfg, seed=seed), strict=True)
        return m.to(BF).cuda()

    def cnet(seed):
        cn = ControlNet(1, dim=cfg["dim"], num_heads=cfg["num_heads"], ffn_dim=cfg["ffn_dim"])
        cn.load_state_dict(gi.controlnet_sd(cfg, 1, seed=seed), strict=True)
        return cn.to(BF).cuda()

    pipe = WanVideoPipeline.from_modules(expert(41), expert(43), cnet(42), cnet(44))
    g = torch.Generator().manual_seed(77)
    shape = (1, 16, GRID[0], 2 * GRID[1], 2 * GRID[2])
    inp = dict(latents=torch.randn(shape, generator=g).to(BF).cuda(), y=torch.randn((1, 20) + shape[2:], generator=g).to(BF).cuda(),
               control=torch.randn(shape, generator=g).to(BF).cuda(),
               posi=torch.randn((1, gi.TINY_CTX_LEN, cfg["text_dim"]), generator=g).to(BF).cuda(),
               nega=torch.randn((1, gi.TINY_CTX_LEN, cfg["text_dim"]), generator=g).to(BF).cuda())

    def run():
        return pipe.denoise(inp["latents"], inp["posi"], inp["nega"], inp["y"], inp["control"], num_inference_steps=3, cfg_scale=5.0,
                            controlnet=True)
    return types.SimpleNamespace(pipe=pipe, run=run, dense=run().clone())


def _log_self_attentions(monkeypatch, pipe):
    """(step, owner, kind) of every self-attention launch of a run, in order: step counted by the pipeline's model_fn calls (two per
    CFG step), owner = the SelfAttention module that is attending, kind = "sparse" / "dense" by the ops wrapper it reached."""
    from goal_force_amd import dit, ops
    log, state = [], {"forwards": 0, "owner": None}
    real_fn, real_attend = pipe.model_fn, dit.SelfAttention.attend

    def model_fn(**kw):
        state["forwards"] += 1
        return real_fn(**kw)

    def attend(self, *a, **k):
        state["owner"] = self
        return real_attend(self, *a, **k)

    def wrap(name, kind):
        real = getattr(ops, name)

        def f(q, k, *a, **kw):
            if q.shape[0] == S and k.shape[0] == S:               # (the cross-attention has 7 keys)
                log.append((((state["forwards"] - 1) // 2) % 3, state["owner"], kind))           # 3 steps per run
            return real(q, k, *a, **kw)
        monkeypatch.setattr(ops, name, f)
    monkeypatch.setattr(pipe, "model_fn", model_fn)
    monkeypatch.setattr(dit.SelfAttention, "attend", attend)
    wrap("flash_attn", "dense")
    wrap("flash_attn_sparse", "sparse")
    return log


def test_pipeline_honours_the_pattern_the_dense_blocks_and_the_dense_steps(pipe_setup, monkeypatch):
    """3 CFG steps with ControlNet on both experts.  An all-selecting pattern and sparse_dense_steps = 3 each reproduce the dense
    latents bit for bit; FrameWindow(1, 1) from the first step differs and is finite; the recorded call list shows which launches
    went to which kernel."""
    from goal_force_amd import dit
    from goal_force_amd.sparse_attention import FrameWindow
    s, pipe = pipe_setup, pipe_setup.pipe
    log = _log_self_attentions(monkeypatch, pipe)
    assert torch.equal(s.run(), s.dense) and log and all(kind == "dense" for *_, kind in log)
    n_dense_run = len(log)
    first_blocks = {m.blocks[0].self_attn for m in (pipe.dit, pipe.dit2, pipe.controlnet.controlnet_dit, pipe.controlnet2.controlnet_dit)}
    try:
        del log[:]
        dit.enable_sparse_attention(pipe, FrameWindow(10))
        assert torch.equal(s.run(), s.dense)
        assert len(log) == n_dense_run and all(kind == "sparse" for *_, kind in log)

        fw = FrameWindow(1, 1)
        assert fw(GRID).density < 0.7
        del log[:]
        dit.enable_sparse_attention(pipe, fw)
        pipe.sparse_dense_steps = 3
        assert torch.equal(s.run(), s.dense) and all(kind == "dense" for *_, kind in log)

        del log[:]
        pipe.sparse_dense_steps = 0
        lat = s.run()
        assert not torch.equal(lat, s.dense) and bool(torch.isfinite(lat.float()).all())
        assert all(kind == "sparse" for *_, kind in log)
        print(f"FrameWindow(1,1), 3 steps, tiny experts: latents rel-L2 from dense {rel_l2(lat, s.dense):.3e}")

        del log[:]
        pipe.sparse_dense_steps = 2
        dit.enable_sparse_attention(pipe, fw, dense_blocks=1)
        lat2 = s.run()
        assert len(log) == n_dense_run and {step for step, *_ in log} == {0, 1, 2}
        for step, owner, kind in log:
            want = "sparse" if step >= 2 and owner not in first_blocks else "dense"
            assert kind == want, (step, kind)
        assert {kind for step, _, kind in log if step == 2} == {"sparse", "dense"}
        assert not torch.equal(lat2, s.dense) and not torch.equal(lat2, lat)
    finally:
        pipe.sparse_dense_steps = 0
        dit.enable_sparse_attention(pipe, None)
    del log[:]
    assert torch.equal(s.run(), s.dense) and all(kind == "dense" for *_, kind in log)
