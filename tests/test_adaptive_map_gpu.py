"""Mass-cover block maps on the GPU (gf_block_map.hip, ops.block_means / block_map_scores / block_map_select / block_map_from_qk,
sparse_attention.MassCover): the stages against the fp64 restatement of the recipe (tests/adaptive_map_refs.py), each with the
bound its arithmetic gives; the selection exactly on scores whose weights are powers of two; the CSR contract on every map; the
sparse kernel reading a device-born map bit for bit as it reads the same map uploaded from the host; the module switch."""
import math
import types

import pytest
import torch

import adaptive_map_refs as ar
import gen_inputs as gi
import sparse_refs as sr

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SHAPES = {"2048": (2048, 2048), "2100": (2100, 2100), "cross": (600, 2085)}     # 2100: a ragged query block AND a ragged tile of 52
LN2 = math.log(2.0)


def check_csr(bm, heads):
    """The contract gf_flash_attn_fwd_vt32_sparse relies on, for a map born on the device; returns its mask."""
    rp = bm.row_ptr.cpu().long()
    assert bm.n_maps == heads and rp.numel() == heads * bm.n_qblocks + 1 and int(rp[0]) == 0
    counts = rp[1:] - rp[:-1]
    assert int(counts.min()) >= 2 and int(counts.max()) <= bm.n_tiles
    idx = bm.tile_idx[: int(rp[-1])].cpu().long()
    assert int(idx.min()) >= 0 and int(idx.max()) < bm.n_tiles
    inner = torch.ones(idx.numel(), dtype=torch.bool)
    inner[rp[1:-1]] = False                                        # the first index of every row but row 0
    assert bool((idx[1:] > idx[:-1])[inner[1:]].all()), "indices ascend inside every row"
    assert bm.head_map.cpu().tolist() == list(range(heads))
    mask = bm.mask()
    assert mask.shape == (heads, bm.n_qblocks, bm.n_tiles) and torch.equal(mask.sum(2).reshape(-1), counts)
    row_ptr, tile_idx = ar.csr(mask)
    assert torch.equal(row_ptr, bm.row_ptr.cpu()) and torch.equal(tile_idx, bm.tile_idx[: int(rp[-1])].cpu())
    return mask


@pytest.fixture(scope="module")
def data():
    """q, k, v per (heads, shape), as column slices of wider buffers (row strides), uploaded once.  q and k carry a per-head common
    component (as trained projections do): the pooled means are then well away from zero, and the scores' error bound — which scales
    with sum |q_mean| |k_mean| — stays above the one rounding of the final `+ log2 n` it does not count."""
    from goal_force_amd import ops
    out = types.SimpleNamespace(ops=ops, t={})
    for heads in (2, 3):
        for name, (sq, skv) in SHAPES.items():
            g = torch.Generator().manual_seed(1000 * heads + sq)
            W = heads * 128
            sign = lambda: (torch.randint(0, 2, (W,), generator=g) * 2 - 1).float()       # noqa: E731
            q = (torch.randn((sq, W), generator=g) + 0.5 * sign()).to(BF)
            k = (torch.randn((skv, W), generator=g) + 0.5 * sign()).to(BF)
            v = torch.randn((skv, W), generator=g).to(BF)
            qbuf = torch.cat([torch.full((sq, 128), 3.0, dtype=BF), q], dim=1).cuda()
            kvbuf = torch.cat([k, v], dim=1).cuda()
            out.t[heads, name] = types.SimpleNamespace(q=q, k=k, v=v, dq=qbuf[:, 128:], dk=kvbuf[:, :W], dv=kvbuf[:, W:], sq=sq, skv=skv,
                                                       n_qb=-(-sq // 256), n_t=-(-skv // 64))
    return out


def always_mask(n_qb, n_t, seed, p=0.15):
    """A seeded static map with at least 2 tiles per row (ops.BlockMap's own contract)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand((n_qb, n_t), generator=g) < p
    for b in range(n_qb):
        m[b, torch.randperm(n_t, generator=g)[:2]] = True
    return m


# ------------------------------------------------------------------ 1, 2: the pooled means and scores
@pytest.mark.parametrize("heads", [2, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_means_against_fp64(data, heads, shape):
    """A mean of n fp32 additions of bf16 values: at most n 2^-24 max|x| from the exact mean (n - 1 roundings of partial sums that
    stay below n max|x|, divided by n), max|x| over the block's column; x 2 for the division's rounding and slack."""
    ops, t = data.ops, data.t[heads, shape]
    for x, dx, block in ((t.q, t.dq, 256), (t.k, t.dk, 64)):
        got = ops.block_means(dx, heads, block).cpu().double()
        ref = ar.block_means(x, heads, block)
        rows = x.shape[0]
        amax = torch.stack([x[r0: r0 + block].double().abs().reshape(-1, heads, 128).amax(0) for r0 in range(0, rows, block)], dim=1)
        err, bound = (got - ref).abs(), 2 * block * 2.0 ** -24 * amax
        print(f"means H={heads} {shape} block {block}: max err {float(err.max()):.3e}, min slack {float((bound - err).min()):.3e}")
        assert got.shape == ref.shape and bool((err <= bound).all())


@pytest.mark.parametrize("heads", [2, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("scale", [None, LN2])
def test_scores_against_fp64_from_the_kernels_own_means(data, heads, shape, scale):
    ops, t = data.ops, data.t[heads, shape]
    qm, km = ops.block_means(t.dq, heads, 256), ops.block_means(t.dk, heads, 64)
    got = ops.block_map_scores(qm, km, t.sq, t.skv, scale=scale).cpu().double()
    ref = ar.scores(qm.cpu(), km.cpu(), t.skv, scale)
    err, bound = (got - ref).abs(), 2 * 128 * 2.0 ** -24 * ar.softmax_c(scale) * ar.abs_dots(qm.cpu(), km.cpu())
    print(f"scores H={heads} {shape} scale {scale}: max err {float(err.max()):.3e}, min bound {float(bound.min()):.3e}")
    assert got.shape == (heads, t.n_qb, t.n_t) and bool((err <= bound).all())


# ------------------------------------------------------------------ 3: the selection, exactly
def exact_rows(n_rows, n_t, forced, seed):
    """Scores whose differences are small integers — every w a power of two, every partial sum exact in fp32 (at most 1024 terms, a
    spread of 12 or 20 binades) — such that no candidate set's mass lies within 1e-4 W of tau W for tau = 0.5, 0.75 (asserted: the
    selection is then decided by the rule, not by a rounding).  Row kinds in turn: random differences 0 .. 12; heavy ties (0 .. 2);
    one dominant tile (the floor); random again on a large negative base."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for r in range(n_rows):
        kind = r % 4
        for attempt in range(200):
            if kind == 1:
                d = torch.randint(0, 3, (n_t,), generator=g)
            elif kind == 2:
                d = torch.full((n_t,), 20)
                d[int(torch.randint(0, n_t, (1,), generator=g))] = 0
            else:
                d = torch.randint(0, 13, (n_t,), generator=g)
            s = (-93.0 if kind == 3 else 3.0) - d.double()
            f = None if forced is None else forced[r % forced.shape[0]]
            if min(ar.threshold_margin(s, tau, f) for tau in (0.5, 0.75)) > 1e-4:
                break
        assert min(ar.threshold_margin(s, tau, f) for tau in (0.5, 0.75)) > 1e-4, (r, n_t)
        rows.append(s)
    return torch.stack(rows)


@pytest.mark.parametrize("with_forced", [False, True])
@pytest.mark.parametrize("n_t", [2, 3, 31, 32, 33, 64, 65, 512, 1024])
def test_selection_is_the_restatements_on_exact_weights(n_t, with_forced):
    from goal_force_amd import ops
    n_qb = 4
    forced = always_mask(n_qb, n_t, seed=n_t) if with_forced else None
    always = ops.BlockMap(forced) if with_forced else None
    for heads in (2, 3):
        s = exact_rows(heads * n_qb, n_t, forced, seed=10 * n_t + heads).reshape(heads, n_qb, n_t)
        ds = s.float().cuda()
        assert torch.equal(ds.cpu().double(), s)
        for tau in (0.5, 0.75, 1.0):
            bm, kept = ops.block_map_select(ds, tau, always=always, want_kept=True)
            got = check_csr(bm, heads)
            want = ar.select(s, tau, forced)
            assert torch.equal(got, want), (n_t, heads, tau, (got != want).nonzero()[:4].tolist())
            want_kept = torch.tensor([[ar.kept_share(s[h, b], want[h, b]) for b in range(n_qb)] for h in range(heads)])
            # exact sums, one fp32 division: within an ulp of the fp64 quotient
            assert float((kept.cpu().double() - want_kept).abs().max()) <= 2.0 ** -23
            if tau == 1.0:
                assert bool(got.all())
        floor_rows = ar.select(s, 0.5, forced).sum(2) == 2
        assert with_forced or n_t == 2 or bool(floor_rows.any()), "the two-tile floor must be active somewhere"


# ------------------------------------------------------------------ 4, 5, 7: maps from random q / k
def assert_selection_properties(s, mask, tau, forced):
    """From the read-back fp32 scores, in fp64; 1e-4 covers a 1024-term fp32 sum (1024 2^-24 = 6.1e-5) plus the exponential's ulp."""
    H, n_qb, n_t = s.shape
    for h in range(H):
        for b in range(n_qb):
            w, W = ar.weights(s[h, b])
            sel = mask[h, b]
            f = torch.zeros(n_t, dtype=torch.bool) if forced is None else forced[b]
            free = sel & ~f
            assert bool(sel[f].all())
            unsel = ~sel
            if bool(free.any()) and bool(unsel.any()):
                assert float(w[free].min()) >= float(w[unsel].max()), (h, b, "the non-forced selected tiles are a top set")
            kept = float(w[sel].sum() / W)
            assert kept >= tau - 1e-4, (h, b, kept)
            if int(sel.sum()) > 2 and bool(free.any()):             # neither the floor nor the forced set holds the row
                group = free & (w == w[free].min())
                without = float((w[sel].sum() - w[group].sum()) / W)
                assert without < tau + 1e-4, (h, b, without, "a smaller top set would have reached the mass")


@pytest.mark.parametrize("heads", [2, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_maps_from_random_operands_have_the_recipes_properties(data, heads, shape):
    """Flat logits (q as it is) and peaky ones (q x 8), with and without forced tiles, tau 0.5 / 0.9; determinism; the staged calls
    against the one call; the CSR contract of every map."""
    ops, t = data.ops, data.t[heads, shape]
    forced = always_mask(t.n_qb, t.n_t, seed=7)
    always = ops.BlockMap(forced)
    densities = {}
    for gain in (1, 8):
        dq = t.dq if gain == 1 else (t.dq.float() * gain).to(BF)
        for tau in (0.5, 0.9):
            for f, a in ((None, None), (forced, always)):
                bm, s, kept = ops.block_map_from_qk(dq, t.dk, heads, tau, always=a, want_scores=True)
                mask = check_csr(bm, heads)
                assert_selection_properties(s.cpu().double(), mask, tau, f)
                est = torch.tensor([[ar.kept_share(s[h, b].cpu(), mask[h, b]) for b in range(t.n_qb)] for h in range(heads)])
                assert float((kept.cpu().double() - est).abs().max()) < 1e-4
                if f is None:
                    densities[gain, tau] = bm.density
                # the same call again: the same bits; the staged calls: the same bits
                again = ops.block_map_from_qk(dq, t.dk, heads, tau, always=a)
                qm, km = ops.block_means(dq, heads, 256), ops.block_means(t.dk, heads, 64)
                s2 = ops.block_map_scores(qm, km, t.sq, t.skv)
                staged, kept2 = ops.block_map_select(s2, tau, always=a, want_kept=True)
                nnz = int(bm.row_ptr[-1])
                assert torch.equal(s2.view(torch.int32), s.view(torch.int32)) and torch.equal(kept2.view(torch.int32), kept.view(torch.int32))
                for other in (again, staged):
                    assert torch.equal(other.row_ptr, bm.row_ptr) and torch.equal(other.tile_idx[:nnz], bm.tile_idx[:nnz])
    print(f"H={heads} {shape}: densities without forced tiles {({k: round(v, 3) for k, v in densities.items()})}")
    assert densities[8, 0.9] < densities[1, 0.9] and densities[1, 0.5] < densities[1, 0.9]


# ------------------------------------------------------------------ 6: non-finite scores are data
def test_non_finite_scores_give_full_rows_and_leave_the_others_alone():
    from goal_force_amd import ops
    g = torch.Generator().manual_seed(3)
    s = (torch.randn((2, 4, 33), generator=g) * 3).cuda()
    clean = check_csr(ops.block_map_select(s, 0.5), 2)
    assert not bool(clean.all(dim=2).any())
    bad = s.clone()
    bad[0, 1, 7], bad[1, 0, 32], bad[1, 3, 0] = float("nan"), float("inf"), float("-inf")
    got = check_csr(ops.block_map_select(bad, 0.5), 2)
    hit = torch.zeros((2, 4), dtype=torch.bool)
    hit[0, 1] = hit[1, 0] = hit[1, 3] = True
    assert bool(got[hit].all()) and torch.equal(got[~hit], clean[~hit])


# ------------------------------------------------------------------ 8: the kernel reads a device-born map right
@pytest.mark.parametrize("heads", [2, 3])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sparse_kernel_reads_the_device_map_as_the_host_copy(data, heads, shape):
    ops, t = data.ops, data.t[heads, shape]
    dq = (t.dq.float() * 8).to(BF)
    bm = ops.block_map_from_qk(dq, t.dk, heads, 0.8, always=ops.BlockMap(always_mask(t.n_qb, t.n_t, seed=8)))
    out, lse = ops.flash_attn_sparse(dq, t.dk, t.dv, heads, bm, lse=True)
    assert "_density" not in bm.__dict__, "the unprofiled path must not read the map back"
    mask = check_csr(bm, heads)
    assert 0.05 < float(mask.float().mean()) < 0.9
    host = ops.BlockMap(mask, head_map=list(range(heads)), device="cuda")
    out_h, lse_h = ops.flash_attn_sparse(dq, t.dk, t.dv, heads, host, lse=True)
    assert torch.equal(out.view(torch.int16), out_h.view(torch.int16)) and torch.equal(lse.view(torch.int32), lse_h.view(torch.int32))
    # mass = 1: the full map, hence the dense kernel's bits
    full = ops.block_map_from_qk(dq, t.dk, heads, 1.0)
    assert bool(check_csr(full, heads).all())
    out_f, lse_f = ops.flash_attn_sparse(dq, t.dk, t.dv, heads, full, lse=True)
    dense, dense_lse = ops.flash_attn_lse(dq, t.dk, t.dv, heads)
    assert torch.equal(out_f.view(torch.int16), dense.view(torch.int16)) and torch.equal(lse_f.view(torch.int32), dense_lse.view(torch.int32))
    assert torch.equal(out_f, ops.flash_attn(dq, t.dk, t.dv, heads))
    # with profiling on, the launch is recorded with the selected share of the keys (one read-back, then kept)
    ops.PROFILE_ATTN = prof = []
    try:
        ops.flash_attn_sparse(dq, t.dk, t.dv, heads, bm)
    finally:
        ops.PROFILE_ATTN = None
    assert prof[0][2:] == (t.sq, max(1, round(t.skv * bm.density)), heads) and bm.density == pytest.approx(float(mask.float().mean()))


# ------------------------------------------------------------------ 9: where the estimate is exact, the promise holds
@pytest.mark.parametrize("heads", [2, 3])
def test_retained_mass_reaches_tau_where_the_estimate_is_exact(heads):
    """All queries of a block equal and all keys of a tile equal: the pooled vectors ARE the rows, n 2^s is the tile's true mass, and
    the true retained mass 2^(lse_sparse - lse_dense) must reach tau — up to the bf16 rounding of p inside the kernel's row sums
    (2^-9 per term on both sums: margin 2^-7).  q is pre-scaled (scale = ln 2, c = 1, as the module path calls the kernels), so the
    kernel's `bf16(q c)` is exact; logits q.k of std ~4 log2 units: a minority of the tiles holds 0.9 of the mass."""
    from goal_force_amd import ops
    S, tau = 2100, 0.9
    g = torch.Generator().manual_seed(40 + heads)
    qv = (torch.randn((-(-S // 256), heads * 128), generator=g) * 0.35).to(BF)
    kv = torch.randn((-(-S // 64), heads * 128), generator=g).to(BF)
    q = qv.repeat_interleave(256, dim=0)[:S].contiguous().cuda()
    k = kv.repeat_interleave(64, dim=0)[:S].contiguous().cuda()
    v = torch.randn((S, heads * 128), generator=g).to(BF).cuda()
    assert torch.equal(ops.block_means(q, heads, 256).cpu(), qv.float().reshape(-1, heads, 128).transpose(0, 1))     # exact means
    bm = ops.block_map_from_qk(q, k, heads, tau, scale=LN2)
    mask = check_csr(bm, heads)
    _, lse_s = ops.flash_attn_sparse(q, k, v, heads, bm, scale=LN2, lse=True)
    _, lse_d = ops.flash_attn_lse(q, k, v, heads, scale=LN2)
    retained = torch.exp2(lse_s.double() - lse_d.double()).cpu()
    print(f"H={heads}: density {bm.density:.3f}, true retained mass min {float(retained.min()):.5f} mean {float(retained.mean()):.5f}")
    assert float(mask.float().mean()) < 0.5, "tau = 0.9 must keep a minority of the tiles here"
    assert float(retained.min()) >= tau * (1 - 2.0 ** -7) and float(retained.max()) <= 1 + 2.0 ** -7


# ------------------------------------------------------------------ 10: the module
GRID = (3, 20, 35)               # 2100 tokens: 9 query blocks (the last of 52 rows), 33 tiles (the last of 52 keys)
S = GRID[0] * GRID[1] * GRID[2]


@pytest.fixture(scope="module")
def block():
    from goal_force_amd import dit
    g = torch.Generator().manual_seed(17)
    blk = dit.DiTBlock(False, 256, 2, 512).to(BF)
    for name, p_ in blk.named_parameters():
        p_.data.copy_((torch.randn(p_.shape, generator=g) * (0.06 if p_.dim() == 2 else 0.02)).to(BF))
    for n in (blk.self_attn.norm_q, blk.self_attn.norm_k, blk.cross_attn.norm_q, blk.cross_attn.norm_k):
        n.weight.data.fill_(1.0)
    blk = blk.cuda()
    x, ctx, t_mod = gi.block_inputs(256, S, gi.TINY_CTX_LEN, seed=33)
    rope = dit.RopeTable.from_grid(dit.precompute_freqs_cis_3d(128), *GRID, "cuda")
    return types.SimpleNamespace(blk=blk, rope=rope, dx=x.cuda(), ctx=ctx.cuda(), t_mod=t_mod.cuda())


def test_block_under_a_mass_cover(block):
    from goal_force_amd import dit, ops
    from goal_force_amd.sparse_attention import FrameWindow, MassCover
    b = block
    before = b.blk(b.dx, b.ctx, b.t_mod, b.rope).clone()
    try:
        dit.enable_sparse_attention(b.blk, MassCover(1.0))
        assert torch.equal(b.blk(b.dx, b.ctx, b.t_mod, b.rope), before), "mass = 1 is the unswitched block bit for bit"
        mc = MassCover(0.8, always=FrameWindow(0, 1), keep_last=True)
        dit.enable_sparse_attention(b.blk, mc)
        on = b.blk(b.dx, b.ctx, b.t_mod, b.rope).clone()
        mask = check_csr(mc.last_map, 2)
        sink = FrameWindow(0, 1).mask(GRID)
        assert bool(mask[:, sink].all()) and float(mask.float().mean()) < 1.0
        static = ops.BlockMap(mask, head_map=[0, 1])
        dit.enable_sparse_attention(b.blk, lambda grid: static)
        assert torch.equal(b.blk(b.dx, b.ctx, b.t_mod, b.rope), on), "the device-born map against its host copy as a static pattern"
        assert not torch.equal(on, before)
    finally:
        dit.enable_sparse_attention(b.blk, None)
    assert torch.equal(b.blk(b.dx, b.ctx, b.t_mod, b.rope), before)


def test_block_under_a_mass_cover_refuses_by_name(block):
    from goal_force_amd import dit
    from goal_force_amd._lib import GoalForceError
    from goal_force_amd.sparse_attention import MassCover
    b, sa = block, block.blk.self_attn
    try:
        dit.enable_sparse_attention(b.blk, MassCover(0.9))
        with pytest.raises(GoalForceError, match="no sparse backward"):
            sa.attend(b.dx[0], b.rope, keep={})
        with pytest.raises(GoalForceError, match="sequence parallelism"):
            sa.attend(b.dx[0], b.rope, sp=types.SimpleNamespace(size=2, rank=0))
        with pytest.raises(GoalForceError, match="needs the token grid"):
            sa(b.dx, sr.rope_complex(dit.precompute_freqs_cis_3d(128), *GRID)[:, None, :])      # a caller's complex freqs
        small = dit.RopeTable.from_grid(dit.precompute_freqs_cis_3d(128), 3, 4, 6, "cuda")
        with pytest.raises(GoalForceError, match="at least 2048 tokens"):
            sa.attend(b.dx[0, :72].contiguous(), small)
        dit.enable_sage_attention(b.blk)
        with pytest.raises(GoalForceError, match="enable_sage_attention"):
            sa.attend(b.dx[0], b.rope)
    finally:
        dit.enable_sage_attention(b.blk, False)
        dit.enable_sparse_attention(b.blk, None)
