"""Inputs of the fixed-maximum self-attention tests (test_attn_fixed_max_cpu.py models them on the CPU, test_attn_fixed_max_gpu.py
runs them through kernel 3) and a torch-CPU model of kernel 3's two softmax schedules on one head.

Everything is in the exp2 domain, as the kernel works: q arrives PRE-SCALED, q' = bf16(q c) with c = Q_PRESCALE(128) = fp32(1 /
sqrt 128) x fp32(log2 e), and is attended with scale = ln 2 — what dit.SelfAttention.attend does — so the kernel's own factor is 1, a
score is s = q' . k in log2 units and the fp64 reference is softmax(ln 2 . q' k^T) v with no second rounding of q in between."""
import math

import numpy as np
import torch

BF = torch.bfloat16
D = 128
TILE = 64
C = float(np.float32(np.float32(1.0 / math.sqrt(D)) * np.float32(1.4426950408889634)))     # dit.Q_PRESCALE(128)
SCALE = math.log(2.0)


def random_case(seed, sq, skv, heads, std=1.0):
    """q' [sq, heads*128] (logit std `std`: q ~ N(0, std^2) before the pre-scale), k, v [skv, heads*128] bf16, CPU."""
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn((sq, heads * D), generator=g) * (std * C)).to(BF)
    k = torch.randn((skv, heads * D), generator=g).to(BF)
    v = torch.randn((skv, heads * D), generator=g).to(BF)
    return q, k, v


def head(t, h):
    return t[:, h * D:(h + 1) * D]


def scores(q, k, h):
    """log2-domain scores of head h in fp64, [sq, skv]."""
    return head(q, h).double() @ head(k, h).double().T


def reference(q, k, v, heads):
    """(softmax(ln 2 . q' k^T) v [sq, heads*128], log2-domain log-sum-exp [sq, heads]) in fp64."""
    out, lse = [], []
    for h in range(heads):
        s = scores(q, k, h) * SCALE
        out.append(torch.softmax(s, dim=-1) @ head(v, h).double())
        lse.append(torch.logsumexp(s, dim=-1) / SCALE)
    return torch.cat(out, dim=1), torch.stack(lse, dim=1)


def add_rise(q, k, h, row, key, rise, first_keys=range(TILE)):
    """Query `row` of head h becomes the constant vector 0.5 and key `key` of that head a constant vector t, t chosen so that the
    pair scores `rise` log2 units above the row's maximum over `first_keys` (the tile that sets the fixed maximum).  Returns the
    rise the bf16 data really has (fp64 arithmetic on the rounded values)."""
    head(q, h)[row] = 0.5
    m0 = float(scores(q, k, h)[row, list(first_keys)].max())
    head(k, h)[key] = torch.tensor((m0 + rise) / (0.5 * D)).to(BF)
    s = scores(q, k, h)[row]
    assert key not in first_keys
    return float(s[key] - s[list(first_keys)].max())


WAVE_ROWS = 32


def model(s, v, schedule, quiet=6.0, sum_rounded_p=True, rescale_l=True):
    """Kernel 3's arithmetic for one head on the CPU: fp32 scores `s` [sq, skv] in the exp2 domain, p = bf16(exp2(s - m)), fp32 row
    sums and fp32 O over 64-key tiles.  schedule "running": when a tile's row maximum lies more than `quiet` above m for any of a
    wave's 32 rows (the lazy rescale is a per-wave decision), every row of the wave moves its m up to its tile maximum and
    rescales O and l;  "fixed": m stays tile 0's row maximum.  sum_rounded_p False: the row sum takes the fp32 p before its
    rounding, as kernel 2's does;  rescale_l False: a move of the maximum rescales O alone (a fault that
    tests/attention_fwd_refs.py injects).  Returns (O / l [sq, 128] fp32, l [sq] fp32, m [sq] fp32) — l is
    what the kernel's overflow test looks at."""
    s = s.float()
    v = v.float()
    sq, skv = s.shape
    m = s[:, :TILE].max(dim=1).values
    o = torch.zeros((sq, v.shape[1]), dtype=torch.float32)
    l = torch.zeros((sq,), dtype=torch.float32)
    for t0 in range(0, skv, TILE):
        st = s[:, t0:t0 + TILE]
        if schedule == "running" and t0 > 0:
            d = (st.max(dim=1).values - m).clamp_min(0.0)
            for r0 in range(0, sq, WAVE_ROWS):
                if not bool((d[r0:r0 + WAVE_ROWS] > quiet).any()):
                    d[r0:r0 + WAVE_ROWS] = 0.0
            alpha = torch.exp2(-d)
            o, l, m = o * alpha[:, None], (l * alpha if rescale_l else l), m + d
        p32 = torch.exp2(st - m[:, None])
        p = p32.to(BF).float()
        l = l + (p if sum_rounded_p else p32).sum(dim=1)
        o = o + p @ v[t0:t0 + TILE]
    return o / l[:, None], l, m


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# ---- the cases of the GPU tests: (name, sq, skv, heads, logit std)
RANDOM = [("std1", 300, 2100, 3, 1.0), ("std3", 257, 2048, 1, 3.0), ("std8", 290, 2560, 2, 8.0)]
# (name, key, rise): the middle of the sweep (tile 15, a steady phase) and the ragged last tile (skv = 2100: keys 2048 .. 2099)
RISES = [("mid60", 1000, 60.0), ("mid90", 1000, 90.0), ("last60", 2090, 60.0), ("last90", 2090, 90.0)]
RISE_SHAPE = (300, 2100, 2)          # sq, skv, heads; the query is row 270 (second query block) of head 1
RISE_ROW, RISE_HEAD = 270, 1
OVERFLOW_RISE = 135.0


def rise_case(key, rise, seed=11):
    sq, skv, heads = RISE_SHAPE
    q, k, v = random_case(seed, sq, skv, heads)
    got = add_rise(q, k, RISE_HEAD, RISE_ROW, key, rise)
    return q, k, v, got


def negative_start_case():
    """Every score of query row 7 / head 0 in the first three tiles far below zero: the fixed maximum is negative."""
    q, k, v = random_case(5, 200, 2560, 2)
    head(q, 0)[7] = 0.5
    head(k, 0)[:192] = -0.5                    # s = -32 there; the later keys score around 0 +- 17
    return q, k, v


def all_equal_case():
    q, k, v = random_case(6, 200, 2560, 2)
    k[:] = 0
    return q, k, v


def huge_then_small_case():
    """The first tile dominates row 7 of both heads: everything after it underflows against the fixed maximum."""
    q, k, v = random_case(7, 200, 2560, 2)
    q[7] = 0.5
    k[:TILE] = 3.0                             # s = 192 for row 7 on the first tile, +-17 afterwards
    return q, k, v
