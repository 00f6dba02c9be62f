"""The coherence gate of the mass-cover maps on the GPU (gf_block_means_coh, gf_block_map_select_gated, gf_block_map_from_qk_gated;
ops.block_means_coherence / block_map_select / block_map_from_qk; sparse_attention.MassCover's thresholds): the statistic against its
fp64 restatement (tests/coherence_refs.py) within the bound its arithmetic gives, the gated selection exactly on power-of-two weights,
null coherences against the ungated entries bit for bit, the one call against the staged calls, the guarantee on operands that meet
its assumptions, the refusals, and the module switch."""
import types

import pytest
import torch

import adaptive_map_refs as ar
import coherence_refs as cr
import gen_inputs as gi

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN, INF = float("nan"), float("inf")


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_map(a, b):
    nnz = int(a.row_ptr[-1])
    return torch.equal(a.row_ptr, b.row_ptr) and torch.equal(a.tile_idx[:nnz], b.tile_idx[:nnz]) and torch.equal(a.head_map, b.head_map)


def check_csr(bm, heads):
    """The contract gf_flash_attn_fwd_vt32_sparse relies on; returns the map's mask."""
    rp = bm.row_ptr.cpu().long()
    assert bm.n_maps == heads and rp.numel() == heads * bm.n_qblocks + 1 and int(rp[0]) == 0
    counts = rp[1:] - rp[:-1]
    assert int(counts.min()) >= 2 and int(counts.max()) <= bm.n_tiles
    assert bm.head_map.cpu().tolist() == list(range(heads))
    mask = bm.mask()
    row_ptr, tile_idx = ar.csr(mask)
    assert torch.equal(row_ptr, bm.row_ptr.cpu()) and torch.equal(tile_idx, bm.tile_idx[: int(rp[-1])].cpu())
    return mask


# ------------------------------------------------------------------------------------------------ 1: coherence against fp64
ROWS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513)
CLASSES = ("equal", "zero", "halves", "onehot", "std1", "offset", "nan", "inf")


def class_rows(kind, rows, heads, block, g):
    """x [rows, heads*128] bf16 of one data class; "halves" and "onehot" are laid out per run of `block` rows."""
    W = heads * 128
    i = torch.arange(rows)
    if kind == "equal":
        return torch.randn((1, W), generator=g).to(BF).repeat(rows, 1)
    if kind == "zero":
        return torch.zeros((rows, W), dtype=BF)
    if kind == "halves":                # the first half of every run +v, the rest -v (an odd run keeps one +v more)
        n = torch.clamp(rows - (i // block) * block, max=block)
        sign = torch.where((i % block) < (n + 1) // 2, 1.0, -1.0)
        return (torch.randn((1, W), generator=g).to(BF).float() * sign[:, None]).to(BF)
    if kind == "onehot":                # row i of a run: 3 at channel i % 128 of every head (orthogonal while the run has <= 128 rows)
        x = torch.zeros((rows, heads, 128))
        x[i, :, (i % block) % 128] = 3.0
        return x.reshape(rows, W).to(BF)
    x = torch.randn((rows, W), generator=g) + (4.0 if kind == "offset" else 0.0)
    if kind in ("nan", "inf"):          # one element of one row, in the last head only
        x[rows // 2, W - 128 + 5] = NAN if kind == "nan" else -INF
    return x.to(BF)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("block", [64, 256])
@pytest.mark.parametrize("heads", [1, 3])
def test_coherence_against_fp64(heads, block, strided):
    """|rho - rho64| <= coherence_refs.coherence_bound(block) (derived there: 191 u for block 256, 71 u for block 64, u = 2^-24) wherever
    the fp64 value is finite; NaN exactly where it is not; the means are ops.block_means's bits; two calls give the same bits."""
    from goal_force_amd import ops
    bound, W = cr.coherence_bound(block), heads * 128
    g = torch.Generator().manual_seed(100 * heads + block)
    worst = 0.0
    for rows in ROWS:
        for kind in CLASSES:
            x = class_rows(kind, rows, heads, block, g)
            if strided:
                buf = torch.full((rows, W + 8), 7.0, dtype=BF)
                buf[:, :W] = x
                dx = buf.cuda()[:, :W]
                assert dx.stride(0) == W + 8
            else:
                dx = x.cuda()
            mean, coh = ops.block_means_coherence(dx, heads, block)
            mean2, coh2 = ops.block_means_coherence(dx, heads, block)
            nb = -(-rows // block)
            assert mean.shape == (heads, nb, 128) and coh.shape == (heads, nb) and coh.dtype == torch.float32
            assert torch.equal(bits(mean), bits(ops.block_means(dx, heads, block))), (rows, kind, "the means are gf_block_means's bits")
            assert torch.equal(bits(mean), bits(mean2)) and torch.equal(bits(coh), bits(coh2)), (rows, kind, "deterministic")
            ref = cr.coherence(x, heads, block)
            got = coh.cpu().double()
            finite = torch.isfinite(ref)
            assert torch.equal(torch.isfinite(got), finite), (rows, kind, got.tolist(), ref.tolist())
            if kind in ("nan", "inf"):
                want_bad = torch.zeros((heads, nb), dtype=torch.bool)
                want_bad[heads - 1, (rows // 2) // block] = True
                assert torch.equal(~finite, want_bad), (rows, kind)
            err = float((got - ref)[finite].abs().max()) if bool(finite.any()) else 0.0
            worst = max(worst, err)
            assert err <= bound, (rows, kind, err, bound)
            if kind == "zero":
                assert bool((got == 1.0).all())
    print(f"coherence H={heads} block {block} strided {strided}: max |rho - rho64| {worst:.3e}, bound {bound:.3e}")


# ------------------------------------------------------------------------------------- 2: the gated selection, exactly
@pytest.mark.parametrize("with_forced", [False, True])
@pytest.mark.parametrize("n_t", [2, 31, 32, 33, 64, 65, 1023, 1024])
def test_gated_selection_is_the_restatements_on_exact_weights(n_t, with_forced):
    """coherence_refs.gate_case: 3 heads whose coherences differ, values exactly at the threshold (pass), one fp32 step below and NaN
    (fire), gate-forced tiles that alone reach mass W, the two-tile floor, query-gated rows (test_coherence_gate_cpu.py asserts the case
    has all of that).  row_ptr, tile_idx, head_map and kept against the restatement."""
    from goal_force_amd import ops
    s, forced, q_coh, k_coh = cr.gate_case(n_t, with_forced)
    always = ops.BlockMap(forced) if with_forced else None
    ds, dq, dk = s.float().cuda(), q_coh.cuda(), k_coh.cuda()
    assert torch.equal(ds.cpu().double(), s)
    for tau in (0.5, 0.75):
        for use_q, use_k in ((True, True), (True, False), (False, True)):
            kw = dict(q_coherence=dq if use_q else None, q_min=cr.GATE_MIN if use_q else None,
                      k_coherence=dk if use_k else None, k_min=cr.GATE_MIN if use_k else None)
            bm, kept = ops.block_map_select(ds, tau, always=always, want_kept=True, **kw)
            got = check_csr(bm, cr.GATE_HEADS)
            want = cr.select_gated(s, tau, forced, q_coh if use_q else None, k_coh if use_k else None, cr.GATE_MIN, cr.GATE_MIN)
            assert torch.equal(got, want), (n_t, tau, use_q, use_k, (got != want).nonzero()[:4].tolist())
            row_ptr, tile_idx = ar.csr(want)
            assert torch.equal(bm.row_ptr.cpu(), row_ptr) and torch.equal(bm.tile_idx[: int(row_ptr[-1])].cpu(), tile_idx)
            # exact sums, one fp32 division: within an ulp of the fp64 quotient; a query-gated row reports 1
            assert float((kept.cpu().double() - cr.kept_gated(s, want)).abs().max()) <= 2.0 ** -23
            if use_q:
                assert kept.cpu()[~(q_coh >= cr.GATE_MIN)].tolist() == [1.0] * 4


# ----------------------------------------------------------------- 3: null coherences are the ungated entries, bit for bit
def random_operands(S, heads, seed):
    """As test_adaptive_map_gpu.py's property test: std 1 plus a per-head common component, column slices of wider buffers."""
    g = torch.Generator().manual_seed(seed)
    W = heads * 128
    sign = lambda: (torch.randint(0, 2, (W,), generator=g) * 2 - 1).float()       # noqa: E731
    q = (torch.randn((S, W), generator=g) + 0.5 * sign()).to(BF)
    k = (torch.randn((S, W), generator=g) + 0.5 * sign()).to(BF)
    qbuf = torch.cat([torch.full((S, 128), 3.0, dtype=BF), q], dim=1).cuda()
    kbuf = torch.cat([k, torch.zeros((S, 8), dtype=BF)], dim=1).cuda()
    return qbuf[:, 128:], kbuf[:, :W]


def raw_select_gated(ops, lib, scores, forced, q_coh, k_coh, mass, q_min, k_min):
    """gf_block_map_select_gated itself (the Python wrapper sends a call without thresholds to the ungated entry)."""
    heads, n_qb, n_t = scores.shape
    ws = torch.empty((int(lib.gf_block_map_select_workspace_bytes(n_qb, n_t, heads)),), dtype=torch.uint8, device="cuda")
    row_ptr, tile_idx, head_map = ops._block_map_out(heads, n_qb, n_t, scores.device)
    kept = torch.empty((heads, n_qb), dtype=torch.float32, device="cuda")
    p = ops._ptr
    status = lib.gf_block_map_select_gated(p(scores), p(forced), p(q_coh), p(k_coh), p(row_ptr), p(tile_idx), p(head_map), p(kept), p(ws),
                                           n_qb, n_t, heads, mass, q_min, k_min, ops._stream(scores))
    return status, ops.BlockMap.from_device(row_ptr, tile_idx, head_map, heads, n_qb, n_t), kept


@pytest.mark.parametrize("heads", [2, 3])
@pytest.mark.parametrize("S", [128, 2100])
def test_null_coherences_are_the_ungated_entries_bit_for_bit(S, heads):
    from goal_force_amd import _lib, ops
    lib = _lib.load()
    dq, dk = random_operands(S, heads, seed=1000 * heads + S)
    n_qb, n_t = -(-S // 256), -(-S // 64)
    forced = cr.always_mask(n_qb, n_t, seed=7)
    for tau in (0.5, 0.9):
        for always in (None, ops.BlockMap(forced)):
            old, s_old, kept_old = ops.block_map_from_qk(dq, dk, heads, tau, always=always, want_scores=True)
            check_csr(old, heads)
            # the Python layer with both thresholds None: the old entries, hence the staged old calls' bits
            qm, km = ops.block_means(dq, heads, 256), ops.block_means(dk, heads, 64)
            staged, kept_st = ops.block_map_select(ops.block_map_scores(qm, km, S, S), tau, always=always, want_kept=True,
                                                   q_coherence=None, k_coherence=None, q_min=None, k_min=None)
            assert same_map(staged, old) and torch.equal(bits(kept_st), bits(kept_old))
            assert same_map(ops.block_map_from_qk(dq, dk, heads, tau, always=always, q_min=None, k_min=None), old)
            # the gated selection entry with null coherences
            fbits = None if always is None else always.forced_bits(dq.device)
            status, raw, kept_raw = raw_select_gated(ops, lib, s_old, fbits, None, None, tau, 0.75, 0.75)
            assert status == 0 and same_map(raw, old) and torch.equal(bits(kept_raw), bits(kept_old))
            # the gated one call with both sides off (thresholds None, coherences asked for)
            off, s_off, kept_off, q_coh, k_coh = ops.block_map_from_qk(dq, dk, heads, tau, always=always, want_scores=True, want_coherence=True)
            assert same_map(off, old) and torch.equal(bits(s_off), bits(s_old)) and torch.equal(bits(kept_off), bits(kept_old))
            assert q_coh.shape == (heads, n_qb) and k_coh.shape == (heads, n_t)
    # random rows are incoherent: rho ~ 1 / n + the common component's share
    assert float(k_coh.max()) < 0.5 and (S < 256 or float(q_coh[:, :-1].max()) < 0.5)


# ------------------------------------------------------------------------------------ 4: one call equals the staged calls
@pytest.fixture(scope="module")
def guarantee():
    """The operands of item 5 on the device, per (runs, heads), uploaded once."""
    out = {}
    for runs in cr.GUARANTEE_RUNS:
        for heads in (2, 3):
            q, k, v = cr.guarantee_operands(*runs, heads)
            out[runs, heads] = types.SimpleNamespace(q=q, k=k, v=v, dq=q.cuda(), dk=k.cuda(), dv=v.cuda())
    return out


@pytest.mark.parametrize("heads", [2, 3])
def test_one_call_equals_the_staged_calls(guarantee, heads):
    from goal_force_amd import ops
    S = cr.GUARANTEE_S
    n_qb, n_t = -(-S // 256), -(-S // 64)
    always = ops.BlockMap(cr.always_mask(n_qb, n_t, seed=11))
    rq, rk = random_operands(S, heads, seed=77 + heads)
    mixed_q = torch.cat([guarantee[(384, 160), heads].dq[:1100], rq[1100:]]).contiguous()      # coherent and incoherent blocks in one map
    cases = [(guarantee[(384, 160), heads].dq, guarantee[(384, 160), heads].dk), (mixed_q, guarantee[(256, 160), heads].dk), (rq, rk)]
    for dq, dk in cases:
        for q_min, k_min, a in ((0.75, 0.75, None), (0.5, None, always), (None, 0.9, always), (1.0, 1.0, None)):
            bm, s, kept, q_coh, k_coh = ops.block_map_from_qk(dq, dk, heads, 0.9, always=a, scale=cr.LN2, q_min=q_min, k_min=k_min,
                                                              want_scores=True, want_coherence=True)
            check_csr(bm, heads)
            again = ops.block_map_from_qk(dq, dk, heads, 0.9, always=a, scale=cr.LN2, q_min=q_min, k_min=k_min)
            assert same_map(again, bm), "two calls, the same bits (the coherences then live in the workspace)"
            qm, qc = ops.block_means_coherence(dq, heads, 256)
            km, kc = ops.block_means_coherence(dk, heads, 64)
            s2 = ops.block_map_scores(qm, km, S, S, scale=cr.LN2)
            staged, kept2 = ops.block_map_select(s2, 0.9, always=a, want_kept=True, q_coherence=None if q_min is None else qc, q_min=q_min,
                                                 k_coherence=None if k_min is None else kc, k_min=k_min)
            assert torch.equal(bits(q_coh), bits(qc)) and torch.equal(bits(k_coh), bits(kc))
            assert torch.equal(bits(s2), bits(s)) and torch.equal(bits(kept2), bits(kept)) and same_map(staged, bm)


# ---------------------------------------------------------------------------------------------------- 5: the guarantee
@pytest.mark.parametrize("heads", [2, 3])
@pytest.mark.parametrize("runs", cr.GUARANTEE_RUNS)
def test_gated_map_keeps_the_mass_where_its_assumptions_hold(guarantee, runs, heads):
    """q constant over runs of q_run tokens, k over runs of k_run keys: every block / tile that does not straddle two runs has equal rows,
    the straddling ones (rho 0.44 .. 0.56) are exactly what thresholds of 0.75 gate — so every row's TRUE retained mass
    2^(lse_sparse - lse_dense) must reach mass, up to the bf16 rounding of p inside the kernel's row sums (margin 2^-7, as
    test_adaptive_map_gpu.py's exact-estimate test); the ungated map on the same operands does not (in fp64: a minimum of 0.02 .. 0.76,
    test_coherence_gate_cpu.py), which is what this test has to catch."""
    from goal_force_amd import ops
    t = guarantee[runs, heads]
    tau, thr, bar = cr.GUARANTEE_MASS, cr.GUARANTEE_MIN, cr.GUARANTEE_MASS * (1 - 2.0 ** -7)
    _, lse_d = ops.flash_attn_lse(t.dq, t.dk, t.dv, heads, scale=cr.LN2)

    def retained(bm):
        _, lse_s = ops.flash_attn_sparse(t.dq, t.dk, t.dv, heads, bm, scale=cr.LN2, lse=True)
        return torch.exp2(lse_s.double() - lse_d.double()).cpu()

    gated, q_coh, k_coh = ops.block_map_from_qk(t.dq, t.dk, heads, tau, scale=cr.LN2, q_min=thr, k_min=thr, want_coherence=True)
    plain = ops.block_map_from_qk(t.dq, t.dk, heads, tau, scale=cr.LN2)
    mask = check_csr(gated, heads)
    r_gated, r_plain = retained(gated), retained(plain)
    print(f"runs {runs} H={heads}: ungated min {float(r_plain.min()):.4f} density {plain.density:.3f}; gated min {float(r_gated.min()):.4f} "
          f"mean {float(r_gated.mean()):.4f} density {gated.density:.3f}")
    sq, sk = cr.straddling(t.q, 256), cr.straddling(t.k, 64)
    assert torch.equal(~(q_coh.cpu() >= thr), sq.expand(heads, -1)), "the straddling query blocks are exactly the gated ones"
    assert torch.equal(~(k_coh.cpu() >= thr), sk.expand(heads, -1)), "the straddling key tiles are exactly the gated ones"
    assert bool(mask[:, sq].all()) and bool(mask[:, :, sk].all()) and float(mask.float().mean()) < 0.7
    assert float(r_gated.min()) >= bar and float(r_gated.max()) <= 1 + 2.0 ** -7
    assert float(r_plain.min()) < bar, "the ungated map must miss the bar here, or this test catches nothing"


# ---------------------------------------------------------------------------------------------------- 6: the refusals
def test_refusals_by_message_leave_the_outputs_untouched():
    from goal_force_amd import _lib, ops
    from goal_force_amd._lib import GoalForceError
    lib, p = _lib.load(), ops._ptr
    heads, S = 2, 256
    dq, dk = random_operands(S, heads, seed=5)
    n_qb, n_t = 1, 4
    st = ops._stream(dq)
    err = lambda: lib.gf_last_error().decode()                                    # noqa: E731
    # gf_block_means_coh: a null coh, and what gf_block_means refuses
    mean = torch.full((heads, n_t, 128), 5.0, device="cuda")
    coh = torch.full((heads, n_t), 5.0, device="cuda")
    qco = torch.full((heads, n_qb), 5.0, device="cuda")
    assert lib.gf_block_means_coh(p(dk), dk.stride(0), p(mean), None, S, heads, 64, st) == -1 and "null pointer (coh)" in err()
    assert lib.gf_block_means_coh(p(dk), dk.stride(0), p(mean), p(coh), S, heads, 128, st) == -1 and "expected block 256" in err()
    assert lib.gf_block_means_coh(p(dk), heads * 128 - 8, p(mean), p(coh), S, heads, 64, st) == -1 and "row stride" in err()
    assert lib.gf_block_means(p(dk), dk.stride(0), p(mean), S, heads, 128, st) == -1 and "expected block 256" in err()
    # the selection: thresholds outside (0, 1] and NaN, by name
    s = torch.randn((heads, n_qb, n_t), device="cuda")
    qc, kc = torch.ones((heads, n_qb), device="cuda"), torch.ones((heads, n_t), device="cuda")
    row_ptr, tile_idx, head_map = (torch.full_like(t, -7) for t in ops._block_map_out(heads, n_qb, n_t, dq.device))
    kept = torch.full((heads, n_qb), 5.0, device="cuda")
    ws = torch.zeros((int(lib.gf_block_map_gated_workspace_bytes(S, S, heads)) + 256,), dtype=torch.uint8, device="cuda")
    for bad in (0.0, -0.5, 1.0001, NAN, INF):
        for q_min, k_min, name in ((bad, 0.5, "q_min"), (0.5, bad, "k_min")):
            assert lib.gf_block_map_select_gated(p(s), None, p(qc), p(kc), p(row_ptr), p(tile_idx), p(head_map), p(kept), p(ws), n_qb, n_t,
                                                 heads, 0.9, q_min, k_min, st) == -1
            assert f"expected {name} in (0, 1]" in err()
    # the one call: NaN and > 1 (<= 0 switches a side off there), a misaligned workspace, a bad mass — before the first launch
    args = lambda w, q_min, k_min, mass=0.9: (p(dq), dq.stride(0), p(dk), dk.stride(0), None, p(row_ptr), p(tile_idx), p(head_map), None,   # noqa: E731
                                              p(kept), p(qco), p(coh), w, S, S, heads, 0.1, mass, q_min, k_min, st)
    for q_min, k_min, msg in ((NAN, 0.5, "q_min in (0, 1]"), (0.5, 1.5, "k_min in (0, 1]"), (0.5, NAN, "k_min in (0, 1]")):
        assert lib.gf_block_map_from_qk_gated(*args(p(ws), q_min, k_min)) == -1 and msg in err()
    assert lib.gf_block_map_from_qk_gated(*args(p(ws) + 16, 0.5, 0.5)) == -1 and "256-byte aligned workspace of gf_block_map_gated_workspace_bytes" in err()
    assert lib.gf_block_map_from_qk_gated(*args(None, 0.5, 0.5)) == -1 and "256-byte aligned workspace" in err()
    assert lib.gf_block_map_from_qk_gated(*args(p(ws), 0.5, 0.5, mass=0.0)) == -1 and "mass share" in err()
    torch.cuda.synchronize()
    assert bool((mean == 5.0).all()) and bool((coh == 5.0).all()) and bool((qco == 5.0).all()) and bool((kept == 5.0).all())
    assert bool((row_ptr == -7).all()) and bool((tile_idx == -7).all()) and bool((head_map == -7).all())
    # the Python layer: a workspace that is too small or misaligned, coherences of the wrong shape, dtype or device, thresholds
    need = int(lib.gf_block_map_gated_workspace_bytes(S, S, heads))
    assert need > int(lib.gf_block_map_workspace_bytes(S, S, heads))
    small = torch.empty((int(lib.gf_block_map_workspace_bytes(S, S, heads)),), dtype=torch.uint8, device="cuda")
    ops.block_map_from_qk(dq, dk, heads, 0.9, workspace=small)                    # enough for the ungated entry
    for w in (small, ws[16: 16 + need]):
        with pytest.raises(GoalForceError, match=rf"block_map_from_qk\.workspace: expected a contiguous, 256-byte aligned uint8 buffer of at least {need}"):
            ops.block_map_from_qk(dq, dk, heads, 0.9, workspace=w, q_min=0.75)
    for bad in (0, 1.5, NAN):
        with pytest.raises(GoalForceError, match=r"block_map_from_qk\.k_min: expected 0 < k_min <= 1"):
            ops.block_map_from_qk(dq, dk, heads, 0.9, k_min=bad)
        with pytest.raises(GoalForceError, match=r"block_map_select\.q_min: expected 0 < q_min <= 1"):
            ops.block_map_select(s, 0.9, q_coherence=qc, q_min=bad)
    sel = lambda **kw: ops.block_map_select(s, 0.9, **kw)                         # noqa: E731
    with pytest.raises(GoalForceError, match=r"block_map_select\.k_coherence: expected contiguous \[2, 4\]"):
        sel(k_coherence=qc, k_min=0.5)
    with pytest.raises(GoalForceError, match=r"block_map_select\.q_coherence: expected contiguous \[2, 1\]"):
        sel(q_coherence=kc, q_min=0.5)
    with pytest.raises(GoalForceError, match=r"block_map_select\.k_coherence: expected dtype torch.float32"):
        sel(k_coherence=kc.double(), k_min=0.5)
    with pytest.raises(GoalForceError, match=r"block_map_select\.k_coherence: tensor must be on the GPU"):
        sel(k_coherence=kc.cpu(), k_min=0.5)
    with pytest.raises(GoalForceError, match=r"block_map_select\.q_coherence: expected q_coherence and q_min together"):
        sel(q_coherence=qc)
    with pytest.raises(GoalForceError, match=r"block_map_select\.k_coherence: expected k_coherence and k_min together"):
        sel(k_min=0.5)


# ---------------------------------------------------------------------------------------------------- 7: the module
GRID = (3, 20, 35)               # 2100 tokens, as test_adaptive_map_gpu.py's module test
S_MOD = GRID[0] * GRID[1] * GRID[2]


def test_block_under_a_gated_mass_cover():
    from goal_force_amd import dit
    from goal_force_amd.sparse_attention import MassCover
    g = torch.Generator().manual_seed(17)
    blk = dit.DiTBlock(False, 256, 2, 512).to(BF)
    for name, p_ in blk.named_parameters():
        p_.data.copy_((torch.randn(p_.shape, generator=g) * (0.06 if p_.dim() == 2 else 0.02)).to(BF))
    for n in (blk.self_attn.norm_q, blk.self_attn.norm_k, blk.cross_attn.norm_q, blk.cross_attn.norm_k):
        n.weight.data.fill_(1.0)
    blk = blk.cuda()
    x, ctx, t_mod = (t.cuda() for t in gi.block_inputs(256, S_MOD, gi.TINY_CTX_LEN, seed=33))
    rope = dit.RopeTable.from_grid(dit.precompute_freqs_cis_3d(128), *GRID, "cuda")
    try:
        plain = MassCover(0.9, keep_last=True)
        dit.enable_sparse_attention(blk, plain)
        out_plain = blk(x, ctx, t_mod, rope).clone()
        none = MassCover(0.9, keep_last=True, q_coherence=None, k_coherence=None)
        dit.enable_sparse_attention(blk, none)
        assert torch.equal(bits(blk(x, ctx, t_mod, rope)), bits(out_plain)), "both thresholds None: MassCover(0.9)'s bits"
        assert same_map(none.last_map, plain.last_map)
        gated = MassCover(0.9, keep_last=True, q_coherence=0.75, k_coherence=0.75)
        dit.enable_sparse_attention(blk, gated)
        out = blk(x, ctx, t_mod, rope)
        assert bool(torch.isfinite(out.float()).all())
        check_csr(gated.last_map, 2)
        print(f"module: density ungated {plain.last_map.density:.3f}, gated {gated.last_map.density:.3f}")
        assert gated.last_map.density >= plain.last_map.density
        # the refusals of the sparse switch fire under the gated pattern as under any other
        from goal_force_amd._lib import GoalForceError
        sa = blk.self_attn
        with pytest.raises(GoalForceError, match="no sparse backward"):
            sa.attend(x[0], rope, keep={})
        with pytest.raises(GoalForceError, match="sequence parallelism"):
            sa.attend(x[0], rope, sp=types.SimpleNamespace(size=2, rank=0))
        small = dit.RopeTable.from_grid(dit.precompute_freqs_cis_3d(128), 3, 4, 6, "cuda")
        with pytest.raises(GoalForceError, match="at least 2048 tokens"):
            sa.attend(x[0, :72].contiguous(), small)
        dit.enable_sage_attention(blk)
        with pytest.raises(GoalForceError, match="enable_sage_attention"):
            sa.attend(x[0], rope)
    finally:
        dit.enable_sage_attention(blk, False)
        dit.enable_sparse_attention(blk, None)
