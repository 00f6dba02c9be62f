"""fp64 reference, fp32 restatements and the error bounds of the attention forward (goal_force_amd/csrc/gf_attention.hip: kernel 2 and
kernel 3 in its exact, fixed-maximum and block-sparse forms).  Plain helper: CPU tensors in, CPU tensors out, no GPU and no project
import (tests/attn_fixed_max_cases.py, another plain helper, lends its tile-schedule model).  head_dim is 128; q, o are
[Sq, heads*128], k, v [Skv, heads*128], lse [Sq, heads] fp32 in the log2 domain.

* `attn_ref`: per head, fp64 on the bf16 inputs upcast: O = softmax(scale Q K^T) V, the log2-domain lse, and P.  With a last-key
  multiplicity m the keys are WRITTEN OUT (m - 1 further copies of the last k / v row) and the copies' probabilities folded back into
  the last column of P; with a key selection (`sel`, the block-sparse entry points) the softmax runs over the selected keys alone.
  `spread(ref, w)` is sum_j w_ij |V_jd - O_id|; with w = P it is the D the bounds are built from.
* `chain_f32`: each kernel's arithmetic restated in torch in another summation order, kinds
    "k2"    kernel 2: fp32 raw scores, scaled in fp32 by c = fp32(scale) fp32(log2 e), running maximum over 64-key tiles with the
            per-wave lazy rescale, p rounded ONCE to bf16 for O, the row sum taken from the fp32 p BEFORE that rounding (see below),
            one rounding of O;
    "k3"    kernel 3: q' = bf16(fp32(q) c) (the second rounding of q), scores q' . k, the lazy per-wave rescale, the row sum taken
            from the SAME rounded p as O (the ninth d-block against a ones fragment);
    "k3fm"  kernel 3 with the maximum fixed at the first visited tile's row maximum.
  The schedules are attn_fixed_max_cases.model's, not a third copy.  `fault=` injects one of FAULTS.
  tests/test_attention_fwd_refs_cpu.py holds the right chains against the reference through both bounds on every case the GPU test
  runs, and shows that every fault is outside.

THE ELEMENT BOUND, derived and not fitted, u = 2^-8 (bf16's unit roundoff: |fl(x) - x| <= u |x|), no element left out, a non-finite
`got` outside:
      |got - ref| <= u |ref| + u W + 2^-16 rms(ref row of the head)
  kernel 3:  W[i,d] = sum_j P_ij |V_jd - O_id| (1 + s_ij + slop_ij / u)
      numerator and denominator share the rounded p, so p's rounding error eps_j enters as P_ij eps_j (V_jd - O_id), |eps_j| <= u;
      s_ij = 1/2 scale sum_d |Q_id K_jd| is the second rounding of q (a relative perturbation of p_ij, in both numerator and
      denominator); it is 0 when the factor c is exactly 1.0f — the pre-scaled q with scale = ln 2, which the CPU test checks;
      slop_ij = 2^-20 scale sum_d |Q_id K_jd|: the fp32 evaluation of the score (as the backward's slop).
  kernel 2:  W[i,d] = sum_j P_ij |V_jd| + sum_j P_ij |V_jd - O_id| slop_ij / u
  TWO CORRECTIONS of the derivation this bound was first written with (W = sum_j P_ij |V_jd - O_id| (1/2 + s_ij) for both kernels),
  both made because the RIGHT chain fell outside it on the CPU, neither a fitted factor:
   1. the 1/2 of p's rounding is 1.  A rounding to nearest is off by up to u |x| (half an ulp at the bottom of a binade), not u / 2,
      and with few keys nothing averages: at kv_len 7 and on the std3 / std8 / prescaled classes the right chains of both kernels
      had elements at 1.01 - 1.13 of the allowance (kernel 3's at 0.98).  The 1/2 inside s_ij is kept as first written: that term
      is a sum of 128 independent roundings of q's elements, half its worst case is out of reach, and the right chain stays inside
      (worst 0.83 of the allowance, class std8).
   2. kernel 2's row sum is NOT of the rounded p: flash_attn_fwd_kernel2 adds the fp32 exp2 results into l (`rs += pe`) and only
      then rounds them for the PV MFMA.  The rounding of p reaches the numerator alone and enters as P_ij eps_j V_jd, with no
      cancellation against O; the (V - O) form does not cover that wherever V has a common part.  This is the kernel's arithmetic as
      designed and within a rounding of the result, so the bound states it as it is, and `l_from_unrounded_p` is a fault of kernel 3
      only.
THE LSE BOUND, per kernel, because the row sums differ:
      kernel 3:  |lse_got - lse_ref| <= log2e u                           (the row sum of ROUNDED p: each term off by up to u)
                                        + log2e max_j (u s_ij + slop_ij)  (the largest score perturbation of the row)
                                        + 2^-22 |lse_ref| + 2^-16         (fp32: m + log2 l, and the sum's order)
      kernel 2:  the same WITHOUT the first term: its row sum is of the fp32 p (correction 2 above), so nothing in it is rounded to bf16.
  Kernel 3 was first written with log2e u / 2: its right chain reached 1.6 x that on the pre-scaled classes, where a few keys carry
  the row — the same worst case of one rounding as above.  Figures: kernel 2 2.7e-5 log2 units at unit logit std (2^-16 + slop),
  1.4e-4 at std 8, 2.7e-4 on far_* (slop and 2^-22 |lse| at scores of 200) — the right chain reaches 0.095 of it, the kernel on the
  GPU 0.085; a key of weight 1e-3 missing from the row sum is 1.4e-3 log2 units, 50 x the allowance.  Kernel 3 on a pre-scaled q
  5.7e-3; with the second rounding of q its worst case dominates (u s_ij: ~1e-2 at unit logit std, 0.2 at std 8).
THE ROW STATISTIC, for what a worst-case bound cannot see (a row 2 % off, a row sum from the wrong p): the norm of a (row, head)'s 128
deviations from the reference over the root-sum-square of the PREDICTED rounding noise.  A bf16 rounding of x is taken as independent
with relative variance VREL = 2^-18 (3 / (2 ln 2)) / 3 (half an ulp uniform, the significand log-uniform: the kernel rounds exp2(s - m)
whose m is not the reference's, so the ulp of P_ij itself is not known):
      k3:  var_row[i] = sum_j P_ij^2 (VREL + vq_ij + slop_ij^2) |V_j - O_i|^2 + sum_d h(O_id)^2 / 3 + 128 (2^-16 rms)^2
      k2:  var_row[i] = sum_j P_ij^2 (VREL |V_j|^2 + slop_ij^2 |V_j - O_i|^2) + the same two
  vq_ij = ln2^2 sum_d h(q'_id)^2 / 3 K_jd^2, the second rounding of q taken as independent from key to key (it is not where the keys
  share a common vector — far_below / far_above — which over-predicts the noise there: the statistic is blunt on those two with
  kernel 3's plain q).  The threshold is MEASURED, not chosen: ROW_CHAIN_WORST is the worst
  ratio of the right chain over every case the GPU test runs (all_cases()), tests/test_attention_fwd_refs_cpu.py measures and asserts
  it, and the kernels' bar is ROW_BAR = 1.25 x that (summation order, the hardware exp2).  One figure per bound class, so that a
  wider one does not blunt the others.  Measured: kernel 2 1.769 (class std3), kernel 3 with the factor exactly 1 ("k3") 1.720
  (a prescaled tile-edge pair), kernel 3 with the second rounding of q ("k3q") 2.333 (std8, fixed maximum) — held rounded up to the
  next hundredth, 1.77, 1.72, 2.34, and asserted to within 2 % (the CPU's fp32 matmul order may move the last digit); bars 2.21,
  2.15, 2.93.  A ratio above 1 on a right chain is a row whose deviation is
  ONE random variable (one dominant key: a single uniform rounding reaches sqrt(3) of its standard deviation, and more where its
  significand sits low in the binade); k3q's worst rows are of that kind as well (logit std 8: one or two keys carry a row), with
  the second rounding of q on top, which vq takes as independent from key to key while it is one draw per query row.  On the GPU
  the kernels reach the restatements' figures to three digits.
"""
import math
import types

import numpy as np
import torch

import attn_fixed_max_cases as fc

BF = torch.bfloat16
HD = 128
TILE = 64
QBLOCK = 256
U = 2.0 ** -8
ABS = 2.0 ** -16
QHALF = 0.5          # the second rounding of q, as a fraction of its worst case (the docstring)
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
VREL = 2.0 ** -18 * (1.5 / LN2) / 3.0
KINDS = ("k2", "k3", "k3fm")
ROW_CHAIN_WORST = {"k2": 1.77, "k3": 1.72, "k3q": 2.34}      # measured per bound class: the docstring; the CPU test asserts them
ROW_BAR = {k: 1.25 * w for k, w in ROW_CHAIN_WORST.items()}
# fault -> the kinds it applies to
FAULTS = {
    "v_row_5pct": KINDS, "drops_last_key": KINDS, "reads_one_past": KINDS, "vt_group_unswapped": KINDS,
    "l_from_unrounded_p": ("k3", "k3fm"), "rescale_skips_l": ("k2", "k3"), "lse_natural_log": KINDS, "lse_transposed": KINDS,
    "lastmult_on_wrong_key": ("k2",), "row_2pct": KINDS,
}


def factor(scale):
    """c = fp32(scale) x fp32(log2 e) in fp32, as the launchers compute it."""
    return float(np.float32(scale) * np.float32(LOG2E))


# ---------------------------------------------------------------------------------------------------------------------
# the cases shared by the CPU and the GPU test
Q_LENS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 289, 513)
K2_KV = (1, 7, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 257, 320, 385)
K3_KV = (128, 129, 143, 144, 145, 159, 160, 161, 175, 176, 177, 191, 192, 193, 255, 256, 257, 319, 320, 321, 384, 385, 448, 449, 513)


def _covering_pairs(kvs, shift):
    """One query length for every key length; 4 is a unit modulo 15, so 15 consecutive key lengths meet every query length."""
    return [(Q_LENS[(4 * i + shift) % len(Q_LENS)], kv) for i, kv in enumerate(kvs)]


K2_PAIRS = _covering_pairs(K2_KV, 0)
K3_PAIRS = _covering_pairs(K3_KV, 7)
TILE_HEADS = (1, 3)
K2_XCD = [(257, 193, 8), (513, 65, 8), (257, 65, 16), (513, 193, 16)]      # (q_len, kv_len, heads): heads 8 and 16, each with 2 and 3 query blocks
K3_XCD = [(257, 193, 8), (513, 129, 8), (257, 129, 16), (513, 193, 16)]
K3_EDGE_CLASSES = (("std1", 1), ("std1", 3), ("prescaled", 3), ("far_below", 1))      # (class, heads) run at every kernel-3 pair: the docstring of all_cases
CLASS_SHAPE = (289, 161)                                # two query blocks; tiles 0, 1 and a ragged tile of 33 keys
CLASS_HEADS = 2
CLASSES = ("std1", "std3", "std8", "prescaled", "far_below", "far_above", "one_hot", "v_const", "k_zero", "rise_mid", "rise_last")
FAR_BELOW_CONTROL = (289, 192)                          # kv_len % 64 == 0: no ragged tile
RISE_ROW, RISE_HEAD, RISE = 270, 1, 60.0                # the query of the rise classes: second query block, wave 0
RISE_KEYS = {"rise_mid": 100, "rise_last": 150}
OVERFLOW = {"overflow_mid": "rise_mid", "overflow_last": "rise_last"}          # the same query and key, the rise attn_fixed_max_cases.OVERFLOW_RISE
MEM_CASES = [("k2", "std1", 97, 145, 2, 1, None), ("k2", "std1", 65, 97, 2, 3, None)]      # further shapes of the GPU test's surroundings test
ONE_HOT_KEY, ONE_HOT_ROWS = 70, (0, 37, 288)
MULTS = (1, 2, 472)
MULT_KV = (1, 33, 63, 64, 65, 97, 129)                  # 97: the last key sits in the lane half `key + 32` of its tile
MULT_Q, MULT_HEADS = 65, 2
SPARSE_SHAPE = (289, 449, 3)                            # 8 tiles, the last one ragged (1 key); two query blocks
SPARSE_MAPS = ("full", "random", "ends_ragged", "skips_ragged", "one_tile", "two_maps")


def sparse_map(name, sq, skv, heads):
    """(lists, head_map): lists[map][query block] = ascending tile numbers; head_map a list of `heads` map numbers or None."""
    nt, nb = -(-skv // TILE), -(-sq // QBLOCK)
    g = torch.Generator().manual_seed(sum(map(ord, name)) + skv)
    rnd = lambda n: sorted(torch.randperm(nt - 1, generator=g)[:n].tolist())          # noqa: E731  (never the last tile)
    if name == "full":
        return [[list(range(nt)) for _ in range(nb)]], None
    if name == "random":
        return [[rnd(3 + b) + ([nt - 1] if b % 2 else []) for b in range(nb)]], None
    if name == "ends_ragged":
        return [[rnd(2 + b) + [nt - 1] for b in range(nb)]], None
    if name == "skips_ragged":
        return [[rnd(4 - b) for b in range(nb)]], None
    if name == "one_tile":
        return [[[nt - 1] if b == 0 else [2] for b in range(nb)]], None
    if name == "two_maps":
        return [[rnd(3) + [nt - 1] for _ in range(nb)], [rnd(2 + b) for b in range(nb)]], [(h + 1) % 2 for h in range(heads)]
    raise ValueError(name)


def csr(lists):
    """(row_ptr, tile_idx) int32 of sparse_map's lists, rows ordered map * n_qblocks + query block."""
    rp, ti = [0], []
    for m in lists:
        for row in m:
            ti += row
            rp.append(len(ti))
    return torch.tensor(rp, dtype=torch.int32), torch.tensor(ti, dtype=torch.int32)


def selection(lists, head_map, heads, sq, skv):
    """sel[head][query block] = the key indices (ascending) that (head, block) attends to."""
    out = []
    for h in range(heads):
        m = lists[head_map[h] if head_map is not None else 0]
        out.append([torch.cat([torch.arange(t * TILE, min((t + 1) * TILE, skv)) for t in row]) for row in m])
    return out


def all_cases():
    """(kind, class, q_len, kv_len, heads, mult, map) of every case the GPU test holds against the bounds.  Kernel 3's pairs run on
    std1 (heads 1 and 3), and besides on `prescaled` — the production class, whose bound has no s_ij and is ~4 x sharper — and on
    far_below, the one class on which a ragged mask off by one cannot hide (the zero key scores 200 above every real one): so every
    residue of the last tile meets both."""
    out = []
    for kind, pairs, xcd in (("k2", K2_PAIRS, K2_XCD), ("k3", K3_PAIRS, K3_XCD), ("k3fm", K3_PAIRS, K3_XCD)):
        edge = [("std1", h) for h in TILE_HEADS] if kind == "k2" else K3_EDGE_CLASSES
        out += [(kind, c, sq, skv, h, 1, None) for sq, skv in pairs for c, h in edge]
        out += [(kind, "std1", sq, skv, h, 1, None) for sq, skv, h in xcd]
        out += [(kind, c, *CLASS_SHAPE, CLASS_HEADS, 1, None) for c in CLASSES]
        out.append((kind, "far_below", *FAR_BELOW_CONTROL, CLASS_HEADS, 1, None))
    out += [("k2", "std1", MULT_Q, n, MULT_HEADS, m, None) for m in MULTS for n in MULT_KV]
    out += [("k3", c, *CLASS_SHAPE, CLASS_HEADS, 1, None) for c in OVERFLOW] + MEM_CASES      # (the repaired rows are the exact path's)
    out += [(kind, "std1", *SPARSE_SHAPE, 1, name) for kind in ("k3", "k3fm") for name in SPARSE_MAPS]
    return out


def case_seed(name, sq, skv, heads):
    return 100003 * sq + 101 * skv + 7 * heads + sum(map(ord, name))


def case_inputs(name, sq, skv, heads):
    """bf16 (q, k, v) and the softmax scale of one data class:
    std1 / std3 / std8     normal data, logit standard deviation 1 / 3 / 8;
    prescaled              the production call: q' = bf16(q C) with C = attn_fixed_max_cases.C and scale = ln 2 (logit std 3);
    far_below / far_above  every score about 200 log2 units below / above zero (q ~ 3.5 u, k ~ -+3.5 u).  With this plain q the second
                           rounding of q moves every score of a row by ~0.3 log2 units: kernel 3's honest bound is two orders wider
                           than its error here (worst 0.004 of the allowance).  What the classes are for — a key that must not be
                           seen scoring 200 above the real ones — is far outside even so (fault reads_one_past);
    one_hot                pre-scaled data; for three queries of each head one key (tile 1) 60 log2 units above every other;
    v_const                v the same row for every key, logit std 8 (a few keys carry each row): D = 0, the result is that row
                           whatever the probabilities — a row sum that is not the sum of the p in O moves it by whole ulps;
    k_zero                 k = 0: the uniform softmax;
    overflow_mid / _last   the rise classes below with a rise of 135: the fixed maximum overflows, the entry point repairs the workgroup;
    rise_mid / rise_last   pre-scaled data; for query RISE_ROW of head RISE_HEAD one key in tile 1 / in the ragged last tile 60 log2
                           units above tile 0's maximum (attn_fixed_max_cases.add_rise)."""
    g = torch.Generator().manual_seed(case_seed(name, sq, skv, heads))
    D = heads * HD
    rn = lambda n: torch.randn((n, D), generator=g)          # noqa: E731
    q, k, v = rn(sq), rn(skv), rn(skv)
    scale = 1.0 / math.sqrt(HD)
    if name in ("std1", "std3", "std8"):
        a = math.sqrt(float(name[3:]))
        q, k = q * a, k * a
    elif name == "prescaled":
        q, k, scale = q * (3.0 * fc.C), k, fc.SCALE
    elif name in ("far_below", "far_above"):
        q, k = 3.5 + 0.1 * q, (-3.5 if name == "far_below" else 3.5) + 0.1 * k
    elif name == "v_const":
        q, k, v = q * math.sqrt(8.0), k * math.sqrt(8.0), v[:1].expand(skv, D).clone()
    elif name == "k_zero":
        k = torch.zeros_like(k)
    elif name in ("one_hot", "rise_mid", "rise_last") or name in OVERFLOW:
        q, k, v, scale = (q * fc.C).to(BF), k.to(BF), v.to(BF), fc.SCALE
        if name == "one_hot":
            others = [j for j in range(skv) if j != ONE_HOT_KEY]
            for h in range(heads):
                for row in ONE_HOT_ROWS:
                    assert fc.add_rise(q, k, h, min(row, sq - 1), ONE_HOT_KEY, 60.0, first_keys=others) > 59.0
        elif name in OVERFLOW:
            assert fc.add_rise(q, k, RISE_HEAD, RISE_ROW, RISE_KEYS[OVERFLOW[name]], fc.OVERFLOW_RISE) >= 130.0
        else:
            assert fc.add_rise(q, k, RISE_HEAD, RISE_ROW, RISE_KEYS[name], RISE) > RISE - 1.0
    else:
        raise ValueError(name)
    return q.to(BF), k.to(BF), v.to(BF), scale


def embed(t, rows_after, cols_before, cols_after, fill=math.nan):
    """A view of t's values inside a larger buffer filled with `fill`: rows behind it, columns on either side."""
    big = torch.full((t.shape[0] + rows_after, cols_before + t.shape[1] + cols_after), fill, dtype=t.dtype, device=t.device)
    view = big[:t.shape[0], cols_before:cols_before + t.shape[1]]
    view.copy_(t)
    return view


def vt_positions(kv_pad, group):
    """key held at every position of a V^T row.  group 16 (gf_transpose_v): inside 16 keys the order 0-3, 8-11, 4-7, 12-15;
    group 32 (gf_transpose_v32): inside 32 keys position 8 g + i holds key 4 g + i (i < 4) or 16 + 4 g + i - 4 (i >= 4)."""
    pos = torch.arange(kv_pad)
    if group == 16:
        p16 = pos % 16
        return (pos - p16) + ((p16 & 3) | ((p16 & 4) << 1) | ((p16 & 8) >> 1))
    p32 = pos % 32
    g, i = p32 // 8, p32 % 8
    return (pos - p32) + torch.where(i < 4, 4 * g + i, 16 + 4 * g + i - 4)


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 reference
def _heads(t, heads):
    return t.view(t.shape[0], heads, HD).transpose(0, 1)              # [heads, S, 128]


def _flat(t):
    return t.transpose(0, 1).reshape(t.shape[1], -1)                  # [S, heads*128]


def attn_ref(q, k, v, heads, scale, mult=1, sel=None):
    """fp64 o [Sq, heads*128], lse2 [Sq, heads], P [heads, Sq, Skv] (zero on keys outside the selection; the written-out copies of a
    multiple last key folded into the last column); the inputs ride along."""
    sq, skv = q.shape[0], k.shape[0]
    Q, K, V = (_heads(t.double(), heads) for t in (q, k, v))
    if mult > 1:
        K = torch.cat([K, K[:, -1:].expand(heads, mult - 1, HD)], dim=1)
        V = torch.cat([V, V[:, -1:].expand(heads, mult - 1, HD)], dim=1)
    s = scale * (Q @ K.transpose(1, 2))
    if sel is not None:
        keep = torch.zeros((heads, sq, skv), dtype=torch.bool)
        for h in range(heads):
            for b, keys in enumerate(sel[h]):
                keep[h, b * QBLOCK:(b + 1) * QBLOCK, keys] = True
        s = s.masked_fill(~keep, -math.inf)
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    den = e.sum(-1, keepdim=True)
    p = e / den
    o = _flat(p @ V)
    if mult > 1:
        p = torch.cat([p[:, :, :skv - 1], p[:, :, skv - 1:].sum(-1, keepdim=True)], dim=-1)
    lse2 = ((m + torch.log(den)).squeeze(-1) * LOG2E).transpose(0, 1).contiguous()
    return types.SimpleNamespace(q=q, k=k, v=v, heads=heads, scale=scale, mult=mult, sel=sel, o=o, lse2=lse2, P=p, _cache={})


def spread(ref, w):
    """sum_j w_ij |V_jd - O_id|, [heads, Sq, 128] fp64 (w = ref.P: the D of the bounds), in query chunks."""
    V, O = _heads(ref.v.double(), ref.heads), _heads(ref.o, ref.heads)
    out = torch.empty_like(O)
    for i0 in range(0, O.shape[1], 32):
        dev = (V[:, None, :, :] - O[:, i0:i0 + 32, None, :]).abs()                   # [H, 32, Skv, 128]
        out[:, i0:i0 + 32] = (w[:, i0:i0 + 32, :, None] * dev).sum(2)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 restatements, with optional injected faults
def _swap16(n):
    """Key order with keys 4..7 and 8..11 of every 16-group exchanged (n a multiple of 16)."""
    return vt_positions(n, 16)


def chain_f32(q, k, v, heads, scale, kind, mult=1, sel=None, fault=None):
    """(o bf16 [Sq, heads*128], lse fp32 [Sq, heads]) of kernel `kind` restated on the CPU.  Faults:
    v_row_5pct             V row Skv / 2 of head 0 is 5 % too large;
    drops_last_key         key kv_len - 1 is left out;
    reads_one_past         the ragged mask is off by one: kernel 3 sees one zero key (score 0 before the maximum, V^T pad 0),
                           kernel 2 a second copy of the last key (its clamped row);
    vt_group_unswapped     V^T in natural key order inside every 16-group where the P fragment holds keys 4..7 and 8..11 exchanged;
    l_from_unrounded_p     (kernel 3) the row sum from the fp32 p, O from the bf16 p;
    rescale_skips_l        a move of the running maximum rescales O but not the row sum;
    lse_natural_log        lse in natural log;
    lse_transposed         lse written [heads, Sq];
    lastmult_on_wrong_key  (kernel 2) the multiplicity bias lands on key kv_len - 2;
    row_2pct               query row Sq / 2 of head 0 is 2 % too large."""
    assert kind in KINDS and (fault is None or kind in FAULTS[fault]), (kind, fault)
    sq, skv = q.shape[0], k.shape[0]
    c = np.float32(factor(scale))
    Q, K, V = (_heads(t.float(), heads).clone() for t in (q, k, v))
    if fault == "v_row_5pct":
        V[0, skv // 2] *= 1.05
    schedule = "fixed" if kind == "k3fm" else "running"
    o = torch.empty((heads, sq, HD), dtype=torch.float32)
    lse = torch.empty((heads, sq), dtype=torch.float32)
    for h in range(heads):
        if kind == "k2":
            s = Q[h] @ K[h].T                                                        # raw scores
            if mult != 1:
                bias = float(np.float32(np.log2(np.float32(mult))) / c)
                s[:, skv - (2 if fault == "lastmult_on_wrong_key" else 1)] += bias
            s = (s.double() * float(c)).float()
        else:
            s = (Q[h] * float(c)).to(BF).float() @ K[h].T
        vh = V[h]
        for b in range(-(-sq // QBLOCK) if sel is not None else 1):
            rows = slice(b * QBLOCK, min((b + 1) * QBLOCK, sq)) if sel is not None else slice(0, sq)
            sb, vb = (s[rows], vh) if sel is None else (s[rows][:, sel[h][b]], vh[sel[h][b]])
            if fault == "drops_last_key":
                sb, vb = sb[:, :-1], vb[:-1]
            elif fault == "reads_one_past":
                extra_s = sb[:, -1:] if kind == "k2" else torch.zeros((sb.shape[0], 1))
                extra_v = vb[-1:] if kind == "k2" else torch.zeros((1, HD))
                sb, vb = torch.cat([sb, extra_s], dim=1), torch.cat([vb, extra_v], dim=0)
            elif fault == "vt_group_unswapped":
                n16 = -(-sb.shape[1] // 16) * 16
                sb = torch.cat([sb, torch.full((sb.shape[0], n16 - sb.shape[1]), -math.inf)], dim=1)
                vb = torch.cat([vb, torch.zeros((n16 - vb.shape[0], HD))], dim=0)[_swap16(n16)]
            ob, l, m = fc.model(sb, vb, schedule, sum_rounded_p=(kind != "k2") != (fault == "l_from_unrounded_p"),
                                rescale_l=fault != "rescale_skips_l")
            o[h, rows], lse[h, rows] = ob, m + torch.log2(l)
    if fault == "row_2pct":
        o[0, sq // 2] *= 1.02
    lse = lse.transpose(0, 1).contiguous()
    if fault == "lse_natural_log":
        lse = lse * LN2
    if fault == "lse_transposed":
        lse = lse.transpose(0, 1).reshape(sq, heads).contiguous()
    return _flat(o).to(BF), lse


# ---------------------------------------------------------------------------------------------------------------------
# the bounds
def _half_ulp(x):
    """Half a bf16 ulp at |x| (8 significand bits): 2^(floor(log2 |x|) - 8); 0 at 0."""
    m, e = torch.frexp(x)                                                          # |x| = |m| 2^e, 0.5 <= |m| < 1
    return torch.where(m != 0, torch.ldexp(torch.ones_like(x), e - 9), torch.zeros_like(x))


def bound_class(kind, scale):
    """"k2" (row sum from the fp32 p), "k3q" (kernel 3, q rounded a second time) or "k3" (kernel 3, the factor is exactly 1)."""
    assert kind in KINDS
    return "k2" if kind == "k2" else ("k3" if factor(scale) == 1.0 else "k3q")


def bounds(ref, kind):
    """(element allowance [Sq, heads*128], predicted row variance [Sq, heads], lse allowance [Sq, heads]), computed once per class."""
    cls = bound_class(kind, ref.scale)
    if cls in ref._cache:
        return ref._cache[cls]
    H, sc, P = ref.heads, ref.scale, ref.P
    Q, K, V, O = (_heads(t.double(), H) for t in (ref.q, ref.k, ref.v, ref.o))
    absqk = sc * (Q.abs() @ K.abs().transpose(1, 2))                               # scale sum_d |Q K|, [H, Sq, Skv]
    slop = 2.0 ** -20 * absqk
    if cls == "k3q":
        s = QHALF * absqk
        qp = (Q.float() * float(np.float32(factor(sc)))).to(BF).double()
        vq = LN2 ** 2 * ((_half_ulp(qp) ** 2 / 3) @ (K ** 2).transpose(1, 2))
    else:
        s, vq = torch.zeros_like(absqk), torch.zeros_like(absqk)
    dist2 = ((V ** 2).sum(-1)[:, None, :] - 2 * (O @ V.transpose(1, 2)) + (O ** 2).sum(-1)[:, :, None]).clamp_min(0.0)
    if cls == "k2":
        W = P @ V.abs() + spread(ref, P * slop) / U
        var = (P ** 2 * (VREL * (V ** 2).sum(-1)[:, None, :] + slop ** 2 * dist2)).sum(-1)
    else:
        W = spread(ref, P * (1.0 + s + slop / U))
        var = (P ** 2 * (VREL + vq + slop ** 2) * dist2).sum(-1)
    rms = O.pow(2).mean(-1, keepdim=True).sqrt()
    allow = _flat(U * O.abs() + U * W + ABS * rms)
    var = var + (_half_ulp(O) ** 2 / 3).sum(-1) + HD * (ABS * rms.squeeze(-1)) ** 2
    pert = torch.where(P > 0, U * s + slop, torch.zeros_like(slop)).amax(-1)      # over the keys of the softmax
    lse_allow = (0.0 if cls == "k2" else LOG2E * U) + LOG2E * pert + 2.0 ** -22 * ref.lse2.transpose(0, 1).abs() + ABS
    ref._cache[cls] = (allow, var.transpose(0, 1).contiguous(), lse_allow.transpose(0, 1).contiguous())
    return ref._cache[cls]


def measure(got, ref, kind):
    """(elements outside the element bound, worst |got - ref| / allowance, worst row ratio); non-finite -> outside / inf."""
    assert got.shape == ref.o.shape, f"shape {tuple(got.shape)} != {tuple(ref.o.shape)}"
    allow, var, _ = bounds(ref, kind)
    err = (got.double() - ref.o).abs()
    bad = ~(err <= allow)
    inf, zero = torch.full_like(err, math.inf), torch.zeros_like(err)
    ratio = torch.nan_to_num(torch.where(allow > 0, err / allow, torch.where(err > 0, inf, zero)), nan=math.inf, posinf=math.inf)
    e2 = (err ** 2).view(err.shape[0], ref.heads, HD).sum(-1)
    row = torch.nan_to_num(torch.where(var > 0, (e2 / var).sqrt(), torch.where(e2 > 0, inf[:, :ref.heads], zero[:, :ref.heads])),
                           nan=math.inf, posinf=math.inf)
    return int(bad.sum()), float(ratio.max()), float(row.max())


def measure_lse(lse, ref, kind):
    """(rows outside the lse bound, worst |lse - ref| / allowance, worst |lse - ref|)."""
    assert lse.shape == ref.lse2.shape and lse.dtype == torch.float32, (lse.shape, lse.dtype)
    allow = bounds(ref, kind)[2]
    err = (lse.double() - ref.lse2).abs()
    bad = ~(err <= allow)
    fin = lambda t: float(torch.nan_to_num(t, nan=math.inf, posinf=math.inf).max())          # noqa: E731
    return int(bad.sum()), fin(err / allow), fin(err)


def row_bar(kind, scale):
    return ROW_BAR[bound_class(kind, scale)]


def assert_within(got, lse, ref, kind, what):
    """o (and lse unless None) against the bounds; prints what it measures and returns (worst element ratio, worst row ratio)."""
    bar = row_bar(kind, ref.scale)
    n, we, wr = measure(got, ref, kind)
    text = f"{what} [{bound_class(kind, ref.scale)}]: {n}/{got.numel()} elements outside u|ref| + uW + 2^-16 rms, worst {we:.3f} of the " \
           f"allowance; worst row {wr:.3f} x the predicted noise (bar {bar:.3f})"
    fails = []
    if n:
        fails.append(f"{n} of {got.numel()} elements outside the bound (worst {we:.2f}x the allowance)")
    if not wr <= bar:
        fails.append(f"a row's error is {wr:.2f}x the predicted rounding noise (bar {bar:.3f})")
    if lse is not None:
        nl, wl, el = measure_lse(lse, ref, kind)
        text += f"; lse: {nl} outside, worst {wl:.3f} of the allowance ({el:.2e} log2 units)"
        if nl:
            fails.append(f"lse: {nl} of {lse.numel()} outside the bound (worst {wl:.2f}x the allowance, {el:.2e} log2 units)")
    print(text)
    assert not fails, f"{what}: " + "; ".join(fails)
    return we, wr


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
