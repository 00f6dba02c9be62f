"""The coherence statistic and the coherence-gated selection of include/goalforce.h (recipe steps 1b and 3) restated in torch fp64, with
the operands the CPU and the GPU tests of the gate share.  Written from the recipe, not from the kernels; the ungated selection is
adaptive_map_refs's."""
import math

import torch

import adaptive_map_refs as ar

BF = torch.bfloat16
NAN = float("nan")
U = 2.0 ** -24                  # fp32 unit roundoff


# ------------------------------------------------------------------------------------------------------------ the statistic
def coherence(x, num_heads, block):
    """fp64 [heads, ceil(rows / block)]: rho = |m|^2 / e of every run of `block` rows of x [rows, heads*128], m the run's mean row and
    e the mean of its rows' squared norms (a ragged last run uses its own count); 1 where e = 0; NaN where m or e is not finite."""
    rows = x.shape[0]
    x = x.double().reshape(rows, num_heads, 128)
    out = []
    for r0 in range(0, rows, block):
        run = x[r0: r0 + block]
        m = run.mean(dim=0)                                   # [heads, 128]
        e = (run * run).sum(dim=2).mean(dim=0)                # [heads]
        rho = (m * m).sum(dim=1) / e
        rho = torch.where(e == 0, torch.ones_like(rho), rho)
        out.append(torch.where(torch.isfinite(rho) & torch.isfinite(e), rho, torch.full_like(rho, NAN)))
    return torch.stack(out, dim=1)


def coherence_bound(block):
    """|rho_fp32 - rho| for finite input whose squares stay in fp32's range, from the recipe's sum orders (u = 2^-24, g_k = k u).

    e:   every term x^2 is >= 0, so the computed e^ = e (1 + d), |d| <= g_De, De = the roundings on the longest path: block / 16 rows x
         8 fma of one lane's chain, 4 + 2 adds of the two butterflies, 3 adds over the waves, 1 division = block / 2 + 10.
    m:   channel c of the mean is a sum of signed terms through Dm = block / 16 (a lane's rows) + 2 + 3 + 1 (division) roundings:
         |dm_c| <= g_Dm mean_i |x_ic| <= g_Dm sqrt(mean_i x_ic^2), hence |dm| <= g_Dm sqrt(e).
    |m|^2 from m^: | |m^|^2 - |m|^2 | <= 2 |m| |dm| + |dm|^2 <= (2 g_Dm + g_Dm^2) e, because |m|^2 <= e (Cauchy-Schwarz); forming it
         costs 8 more roundings on non-negative terms (a product, a fma, 6 butterfly adds): relative g_8 of a value <= e (1 + 2 g_Dm).
    rho^ = fl(|m^|^2~ / e^): with rho <= 1,  |rho^ - rho| <= (2 g_Dm + g_8 + rho g_De + u) (1 + O(g_De)) <= (2 Dm + 8 + De + 1) u x 1.001.
    Block 256: (44 + 8 + 138 + 1) u = 191 u = 1.14e-5 (below 2^-16); block 64: (20 + 8 + 42 + 1) u = 71 u = 4.3e-6."""
    d_m, d_e = block // 16 + 6, block // 2 + 10
    return (2 * d_m + 8 + d_e + 1) * U * 1.001


# ------------------------------------------------------------------------------------------------------- the gated selection
def _passes(coh, minimum):
    """`coh >= minimum` as the kernel sees it: both fp32; a NaN does not pass."""
    return torch.as_tensor(coh, dtype=torch.float32) >= torch.tensor(minimum, dtype=torch.float32)


def select_gated(s, tau, forced=None, q_coh=None, k_coh=None, q_min=None, k_min=None):
    """bool [heads, n_qb, n_t]: adaptive_map_refs.select with the gate.  A row (h, b) whose q_coh[h][b] does not pass q_min selects every
    tile; a tile t whose k_coh[h][t] does not pass k_min is forced for every row of head h, OR-ed with forced[b].  q_coh / k_coh None:
    that side is off."""
    H, n_qb, n_t = s.shape
    out = torch.zeros((H, n_qb, n_t), dtype=torch.bool)
    for h in range(H):
        k_forced = torch.zeros(n_t, dtype=torch.bool) if k_coh is None else ~_passes(k_coh[h], k_min)
        for b in range(n_qb):
            if q_coh is not None and not bool(_passes(q_coh[h, b], q_min)):
                out[h, b] = True
                continue
            f = k_forced if forced is None else (k_forced | forced[b])
            out[h, b] = ar.select_row(s[h, b], tau, f)
    return out


def kept_gated(s, sel):
    """fp64 [heads, n_qb]: the estimated kept share of every row of a selection (1 for a row that selects everything)."""
    H, n_qb, _ = s.shape
    return torch.tensor([[1.0 if bool(sel[h, b].all()) else ar.kept_share(s[h, b], sel[h, b]) for b in range(n_qb)] for h in range(H)],
                        dtype=torch.float64)


# ------------------------------------------------------------------------- the selection's test case (exact weights, 3 heads)
GATE_HEADS, GATE_QB, GATE_MIN = 3, 4, 0.75
BELOW = float(torch.nextafter(torch.tensor(GATE_MIN, dtype=torch.float32), torch.tensor(0.0)))     # one fp32 step below the threshold


def always_mask(n_qb, n_t, seed, p=0.15):
    """A seeded static map with at least 2 tiles per row (ops.BlockMap's own contract)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand((n_qb, n_t), generator=g) < p
    for b in range(n_qb):
        m[b, torch.randperm(n_t, generator=g)[:2]] = True
    return m


def gate_case(n_t, with_forced):
    """Scores whose weights are powers of two (every fp32 partial sum exact: the selection is decided by the rule, not by a rounding —
    no candidate set's mass within 1e-4 W of tau W for tau = 0.5, 0.75, asserted) under coherences that differ per head:
      k_coh  head 0: about a fifth of the tiles fire — exactly at the threshold (passes), one fp32 step below (fires), NaN (fires), 0.3;
             head 1: exactly ONE tile fires (a NaN), and the dominant tile of its one-dominant-tile row is that tile: the gate-forced
                     tile alone reaches mass W, and without shared forced bits the two-tile floor must add the second;
             head 2: another tenth, other tiles.
      q_coh  per head another set of rows at the threshold / one step below / NaN: a gated row selects everything.
    Row kinds by query block: 0 random differences 0 .. 12; 1 heavy ties (0 .. 2); 2 one dominant tile; 3 random on a large negative base.
    -> (scores fp64 [3, 4, n_t], forced bool [4, n_t] or None, q_coh fp32 [3, 4], k_coh fp32 [3, n_t])."""
    H, n_qb = GATE_HEADS, GATE_QB
    g = torch.Generator().manual_seed(7000 + 10 * n_t + int(with_forced))
    forced = always_mask(n_qb, n_t, seed=n_t) if with_forced else None
    values = torch.tensor([1.0, GATE_MIN, 0.9, BELOW, NAN, 0.3], dtype=torch.float32)
    k_coh = torch.ones((H, n_t), dtype=torch.float32)
    k_coh[0] = values[torch.multinomial(torch.tensor([0.5, 0.15, 0.15, 0.1, 0.05, 0.05]), n_t, replacement=True, generator=g)]
    k_coh[1] = values[torch.multinomial(torch.tensor([0.6, 0.2, 0.2, 0.0, 0.0, 0.0]), n_t, replacement=True, generator=g)]
    lone = int(torch.randint(0, n_t, (1,), generator=g))
    k_coh[1, lone] = NAN
    k_coh[2] = values[torch.multinomial(torch.tensor([0.6, 0.15, 0.15, 0.05, 0.0, 0.05]), n_t, replacement=True, generator=g)]
    q_coh = torch.tensor([[1.0, GATE_MIN, BELOW, NAN], [BELOW, 1.0, 0.9, GATE_MIN], [GATE_MIN, NAN, 1.0, 1.0]], dtype=torch.float32)
    s = torch.zeros((H, n_qb, n_t), dtype=torch.float64)
    for h in range(H):
        k_forced = ~_passes(k_coh[h], GATE_MIN)
        for b in range(n_qb):
            f = k_forced if forced is None else (k_forced | forced[b])
            for attempt in range(400):
                if b == 1:
                    d = torch.randint(0, 3, (n_t,), generator=g)
                elif b == 2:
                    d = torch.full((n_t,), 20)
                    d[lone if h == 1 else int(torch.randint(0, n_t, (1,), generator=g))] = 0
                else:
                    d = torch.randint(0, 13, (n_t,), generator=g)
                row = (-93.0 if b == 3 else 3.0) - d.double()
                if min(ar.threshold_margin(row, tau, f) for tau in (0.5, 0.75)) > 1e-4:
                    break
            assert min(ar.threshold_margin(row, tau, f) for tau in (0.5, 0.75)) > 1e-4, (n_t, h, b)
            s[h, b] = row
    return s, forced, q_coh, k_coh


# -------------------------------------------------------------------------------------------- the guarantee's operands (item 5)
GUARANTEE_S, GUARANTEE_MASS, GUARANTEE_MIN = 2100, 0.9, 0.75
GUARANTEE_RUNS = [(384, 64), (256, 160), (384, 160)]
LN2 = math.log(2.0)


def guarantee_operands(q_run, k_run, heads):
    """q [S, heads*128] bf16 constant over runs of q_run tokens (values of std 0.35: with scale = ln 2 the logits have a std of ~4 log2
    units), k constant over runs of k_run keys, v random.  Runs that are no multiple of the 256-row block / 64-key tile make blocks and
    tiles that straddle two runs: their pooled vector is neither run's."""
    S = GUARANTEE_S
    g = torch.Generator().manual_seed((140 if (q_run, k_run) == (384, 64) else 240) + heads)
    qv = (torch.randn((-(-S // q_run), heads * 128), generator=g) * 0.35).to(BF)
    kv = torch.randn((-(-S // k_run), heads * 128), generator=g).to(BF)
    q = qv.repeat_interleave(q_run, dim=0)[:S].contiguous()
    k = kv.repeat_interleave(k_run, dim=0)[:S].contiguous()
    v = torch.randn((S, heads * 128), generator=g).to(BF)
    return q, k, v


def straddling(x, block):
    """bool [ceil(rows / block)]: the runs of `block` rows whose rows are not all equal."""
    return torch.tensor([bool((x[r0: r0 + block] != x[r0]).any()) for r0 in range(0, x.shape[0], block)])


def map_fp64(q, k, heads, tau, scale, q_min=None, k_min=None):
    """The recipe end to end in fp64 -> (mask bool [heads, n_qb, n_t], q_coh, k_coh fp64)."""
    qm, km = ar.block_means(q, heads, ar.QB), ar.block_means(k, heads, ar.KB)
    s = ar.scores(qm, km, k.shape[0], scale)
    q_coh, k_coh = coherence(q, heads, ar.QB), coherence(k, heads, ar.KB)
    mask = select_gated(s, tau, None, None if q_min is None else q_coh, None if k_min is None else k_coh, q_min, k_min)
    return mask, q_coh, k_coh


def retained_fp64(q, k, heads, mask, scale):
    """fp64 [heads, S]: every query row's true retained softmax mass under `mask` — the share of sum_j 2^(c q.k_j) on the kept tiles."""
    S, Skv = q.shape[0], k.shape[0]
    c = ar.softmax_c(scale)
    qh, kh = q.double().reshape(S, heads, 128), k.double().reshape(Skv, heads, 128)
    logits = c * torch.einsum("ihd,jhd->hij", qh, kh)
    p = torch.exp2(logits - logits.amax(dim=2, keepdim=True))
    keep = mask.repeat_interleave(ar.QB, dim=1)[:, :S].repeat_interleave(ar.KB, dim=2)[:, :, :Skv]
    return (p * keep).sum(dim=2) / p.sum(dim=2)
