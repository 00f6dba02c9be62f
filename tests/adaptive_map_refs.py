"""The mass-cover block-map recipe of include/goalforce.h restated in torch fp64 (means, scores, selection, CSR), for the tests of
gf_block_map.hip / ops.block_map_from_qk / sparse_attention.MassCover.  Written from the recipe, not from the kernels."""
import math

import torch

QB, KB = 256, 64


def block_means(x, num_heads, block):
    """fp64 [heads, ceil(rows / block), 128]: the mean of every run of `block` rows of x [rows, heads*128]; the ragged last run divides
    by its own count."""
    rows = x.shape[0]
    x = x.double().reshape(rows, num_heads, 128)
    return torch.stack([x[r0: r0 + block].mean(dim=0) for r0 in range(0, rows, block)], dim=1)


def softmax_c(scale=None):
    """c = fp32(double(fp32(scale)) * log2(e)), the factor the scores entry forms on the host."""
    scale = 1.0 / math.sqrt(128) if scale is None else scale
    scale32 = float(torch.tensor(scale, dtype=torch.float32))
    return float(torch.tensor(scale32 * 1.4426950408889634, dtype=torch.float64).to(torch.float32))


def tile_keys(kv_len):
    """Keys per tile, fp64 [n_tiles]: 64, or the ragged last tile's count."""
    n_t = -(-kv_len // KB)
    n = torch.full((n_t,), float(KB), dtype=torch.float64)
    n[-1] = kv_len - KB * (n_t - 1)
    return n


def scores(q_mean, k_mean, kv_len, scale=None):
    """fp64 [heads, n_qb, n_t]: c <q_mean, k_mean> + log2(keys of the tile)."""
    dots = torch.einsum("hbd,htd->hbt", q_mean.double(), k_mean.double())
    return softmax_c(scale) * dots + torch.log2(tile_keys(kv_len))


def abs_dots(q_mean, k_mean):
    """sum_d |q_mean_d| |k_mean_d|, fp64 [heads, n_qb, n_t] (the scale of a score's rounding error)."""
    return torch.einsum("hbd,htd->hbt", q_mean.double().abs(), k_mean.double().abs())


def weights(s):
    """(w, W) of one row of scores: w = 2^(s - max s), W = sum w, fp64."""
    s = s.double()
    w = torch.exp2(s - s.max())
    return w, w.sum()


def select_row(s, tau, forced=None):
    """The selection of one row: bool [n_t].  s: scores (log2 domain); forced: bool [n_t] or None."""
    s = torch.as_tensor(s).double()
    n_t = s.numel()
    forced = torch.zeros(n_t, dtype=torch.bool) if forced is None else torch.as_tensor(forced).bool().clone()
    if tau >= 1.0 or not bool(torch.isfinite(s).all()):
        return torch.ones(n_t, dtype=torch.bool)
    w, W = weights(s)
    F = w[forced].sum()
    if F >= tau * W:
        sel = forced.clone()
    else:
        sel = None
        for theta in sorted(set(w.tolist()), reverse=True):          # the largest threshold that reaches the mass
            if F + w[~forced & (w >= theta)].sum() >= tau * W:
                sel = forced | (w >= theta)
                break
        assert sel is not None                                       # theta = min w takes every tile: F + the rest = W
    while int(sel.sum()) < 2:                                        # the floor: the largest unselected w, lowest index on ties
        best = None
        for t in range(n_t):
            if not sel[t] and (best is None or w[t] > w[best]):
                best = t
        sel[best] = True
    return sel


def select(s, tau, forced=None):
    """bool [heads, n_qb, n_t] from scores [heads, n_qb, n_t]; forced: bool [n_qb, n_t] (shared by the heads) or None."""
    H, n_qb, n_t = s.shape
    out = torch.zeros((H, n_qb, n_t), dtype=torch.bool)
    for h in range(H):
        for b in range(n_qb):
            out[h, b] = select_row(s[h, b], tau, None if forced is None else forced[b])
    return out


def csr(mask):
    """(row_ptr int32 [rows + 1], tile_idx int32) of a bool [heads, n_qb, n_t]: rows in (head, block) order, indices ascending."""
    flat = mask.reshape(-1, mask.shape[-1])
    row_ptr = torch.zeros(flat.shape[0] + 1, dtype=torch.int64)
    row_ptr[1:] = flat.sum(1).cumsum(0)
    return row_ptr.to(torch.int32), flat.nonzero()[:, 1].to(torch.int32)


def kept_share(s, sel):
    """sum of the selected w / W of one row, fp64."""
    w, W = weights(s)
    return float(w[sel].sum() / W)


def threshold_margin(s, tau, forced=None):
    """min over the candidate sets (the forced tiles alone, and forced + every top set by value) of |their mass - tau W| / W: how far
    the row is from a selection decided by rounding."""
    w, W = weights(torch.as_tensor(s))
    forced = torch.zeros(w.numel(), dtype=torch.bool) if forced is None else torch.as_tensor(forced).bool()
    F = w[forced].sum()
    gaps = [abs(float(F - tau * W))]
    for theta in set(w.tolist()):
        gaps.append(abs(float(F + w[~forced & (w >= theta)].sum() - tau * W)))
    return min(gaps) / float(W)
