"""fp64 references, fp32 restatements, derived bounds, data classes and case tables of the folded cross-attention
(goal_force_amd/csrc/gf_cross_fold.hip: gf_cross_probs and gf_cross_fold_table).  Plain helper: CPU tensors in, CPU
tensors out, no GPU and no project import.  head_dim is 128; q [Sq, H*128], k, v [n, H*128], w_o [N, H*128], P [Sq, H, n_pad] (the
kernel's [Sq, H*n_pad] viewed per head), U [N, H, n_pad].  `m` is the last key's multiplicity, a float >= 1.

* `probs_ref`: fp64 softmax over [k_0 .. k_{n-2}, k_{n-1} x m] per head -> (p [Sq, H, n], S_abs [Sq, H, n] = sum_d |q_d k_d|).
  `probs_layout(p, n_pad)`: the documented image — bf16(p) in columns < n, bf16(p_last - bf16(p_last)) in column n, zeros after it.
* `table_ref`: fp64 sum_d v[j, h*128+d] w_o[n, h*128+d] in the layout [N, H*n_pad] (column n a copy of column n - 1, zeros after
  it) as a gemm_refs.Ref, so that gemm_refs.judge / assert_pinned hold it with K = 128.
* `probs_f32` / `table_f32`: the two kernels restated in fp32 torch as the header states them.  probs: raw scores Q K^T in fp32, the
  bias log2f(m) / c on the last key's raw score, ONE fma(s, c, -fl(max c)), exp2, the fp32 row sum, its reciprocal, the product, one
  rounding; the residue fma(e_last, 1 / l, -bf16(w_last)) — `wl - bf16(wl)` as the compiler contracts it with wl = pl * inv, the exact
  product less the rounded weight: within half an fp32 ulp of w - bf16(w), and closer to p — rounded once more.  table: 128 sequential fp32 FMAs in d order, one rounding.
  `fault=` injects one of PROBS_FAULTS / TABLE_FAULTS; tests/test_cross_fold_refs_cpu.py shows that the right restatements are inside
  every bar on every input of the GPU test and that every fault is outside a named one.

THE BARS OF P (`judge_probs`), u = 2^-8, no element left out, a non-finite `got` outside:
  element   |got_j - p_j|            <= u p_j + p_j E_j + FLOOR                      (columns j < n)
  last key  |got_{n-1} + got_n - p_last| <= 2^-16 p_last + p_last E_last + FLOOR     (two stacked roundings: the residue r = w - bf16(w)
            is exact in fp32, |r| <= u w, and is rounded once: |bf16(r) - r| <= u |r| <= 2^-16 w)
  row       |sum_{j<=n} got_j - 1|   <= the sum of the row's bounds above (the last key's pair with the last-key bound)
  zeros     columns n + 1 .. n_pad - 1 are +0 bit for bit
  bits      the count of elements (columns < n) whose bf16 bits differ from bf16(fp64 p) is at most gemm_refs.cap(numel, rate) (`bits_cap`: the same
            quantity where the mean is large) with
            rate = 2 x the share the fp32 restatement shows on the same inputs (v_exp_f32 and the MFMA's summation order are not
            torch's fp32).  A restatement that shows no differing element among N says only that the rate is below ~1/N, so the
            count entering the rate is at least 1.
  E_j, the relative error of the kernel's fp32 weight w_j against p_j, FIRST ORDER TERMS SUMMED AND CLOSED WITH expm1 (a product of
  factors (1 + e_i) is at most exp(sum e_i)), times (1 + u) because the rounding to bf16 acts on w, not on p.  In log2 units, with
  c = fp32(scale) fp32(log2 e), S_j = sum_d |q_d k_d|, B = log2 m (the last key only):
      d_j =  128 2^-23 c S_j         the 128-term MFMA sum: exact products, every partial sum <= S_j, one fp32 ulp per addition in
                                     whatever order the instruction adds (gemm_refs' argument)
           + 3 2^-24 c S_j           c itself: scale to fp32, log2 e to fp32, their product
           + 2^-24 (c S_j + B)       the bias add on the raw score (last key)
           + 4 2^-24 B               log2f(m), the division by c, and c again (last key)
           + 2^-24 (c S_j + c S_max + B)   the one rounding of fma(s, c, -mc): |c s_j - mc| <= c S_j + c S_max + B.  fl(max c) itself is
                                     common to all keys of the row and cancels in the normalisation: no term.
      E_j = (1 + u) expm1( ln 2 (d_j + max_k d_k)      the softmax's sensitivity: key j's own exponent and the row sum's, which is a
                                                        p-weighted mean of the d_k and so at most their maximum
                         + 2 2^-23                      one ulp of v_exp_f32, on e_j and (weighted mean again) on the row sum
                         + 64 2^-24                     the <= 64-term row sum of positive terms, any order
                         + 2^-23 + 2^-24 )              the reciprocal (one ulp) and the product
  FLOOR = 2^-126: v_exp_f32 returns 0 for a result below the smallest normal fp32 (it has no denormal results) where the reference
  holds p > 0, and a weight below 2^-126 lands on bf16's denormal grid (spacing 2^-133) — either way the miss is at most p < 2^-126.
  It is on the last-key bar too (one_hot: a cold last key has p = 2^-522 in fp64 and 0 on the device); the issue's form has none
  there and would refuse an exact 0.
THE BARS OF U: exact classes bit for bit; Gaussians gemm_refs' two bars with K = 128 (`table_ref` is a gemm_refs.Ref).
THE BAR OF THE FOLDED PRODUCT (`product_ref`): F^ = P^ U^^T + b formed in fp64 from the device's own P^, U^ against the unfolded
  fp64 function F = sum_h P_h V_h W_o,h^T + b, per element
      |F^ - F| <= sum_{h, j<n-1} p (u + E) |U| + p_last (2^-16 + E_last) |U_last|          (P: its rounding, the residue pair)
                + sum_{h, j<n} p (1 + u + E) (u |U| + 128 2^-23 S_U)                        (U: its rounding, its fp32 sum)
                + FLOOR sum |U|
  CORRECTED from the form this was first asked in, which took U's rounding over the keys j < n - 1 "again": the LAST key's table
  column is rounded to bf16 like every other (both copies of it, identically), the residue pair repairs P's rounding and not U's, and
  on the pad_dominant class that term — u p_last |U_last| — is the largest of all.  The unfolded path makes the same error when it
  rounds O.  S_U = sum_d |v w_o| carries the table's fp32 accumulation (128 additions, one ulp each).
"""
import functools
import math
import types

import numpy as np
import torch

import attention_fwd_refs as A
import gemm_refs as G
from forward_refs import bits, rb

BF = torch.bfloat16
HD = 128
MAXK = 64
U8 = 2.0 ** -8
U16 = 2.0 ** -16
EPS = 2.0 ** -24
FLOOR = 2.0 ** -126
LN2 = math.log(2.0)

PROBS_FAULTS = ("residue_dropped", "residue_shifted", "mult_missing", "mult_on_wrong_key", "mask_drops_last", "mask_reads_one_past",
                "halves_swapped", "d_groups_natural", "max_first_half", "norm_by_rounded_sum", "head_plus_one", "row_2pct")
TABLE_FAULTS = ("table_col_zero", "table_col_from_n_minus_2", "table_bf16_partials", "table_head_slice_off")

# ---------------------------------------------------------------------------------------------------------------------
# the case tables
N_KEYS = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63)
NON_MINIMAL = ((5, 64), (20, 48), (1, 32))
Q_LENS = (1, 31, 32, 33, 127, 128, 129, 257)
HEADS = (1, 3, 8)
MULTS = (1.0, 2.0, 1.5, 472.0, 511.0)
N_OUT = (1, 63, 64, 65, 200)
CLASSES = ("std1", "std3", "std8", "pad_dominant", "pad_negligible", "far_below", "far_above")
CLASS_SHAPES = ((129, 41, 3, 472.0), (33, 33, 1, 472.0))      # (q_len, n_keys, heads, m): the production shape's small twin, and one head
UNIFORM_N = (1, 2, 4, 8, 16, 32)
TABLE_CLASSES = ("integers", "selector", "gauss")
PRODUCT_CASES = (("std3", 129, 41, 8, 472.0), ("pad_dominant", 129, 41, 8, 472.0), ("std3", 33, 33, 8, 472.0),
                 ("pad_dominant", 33, 33, 8, 472.0))


MEM_PROBS = ((129, 41, 48, 3), (33, 33, 64, 1), (257, 5, 16, 8))          # (q_len, n_keys, n_pad, heads) of the GPU test's strided runs (std1, m 472)
MEM_TABLE = ((41, 48, 3, 65), (33, 64, 1, 200), (5, 16, 8, 63))              # (n_keys, n_pad, heads, n_out), gauss
K2_CASES = (("std3", 129, 41, 3, 472), ("std1", 33, 33, 1, 2), ("pad_dominant", 129, 41, 3, 472))


def pad_min(n_keys):
    """The smallest n_pad the ABI takes: n_keys + 1 (the residue column) rounded up to 16."""
    return -(-(n_keys + 1) // 16) * 16


KEY_CASES = tuple((n, pad_min(n)) for n in N_KEYS) + NON_MINIMAL


def _covering_pairs():
    """Two walks over the key cases, 4 query lengths apart (3 is a unit modulo 8): every key case meets two query lengths, every
    query length four key cases — attention_fwd_refs._covering_pairs' idea on the two tables of this file."""
    out = []
    for shift in (0, 4):
        out += [(Q_LENS[(3 * i + shift) % len(Q_LENS)], n, n_pad) for i, (n, n_pad) in enumerate(KEY_CASES)]
    return out


PAIRS = _covering_pairs()                  # (q_len, n_keys, n_pad)


def other_probs_cases():
    """(class, q_len, n_keys, n_pad, heads, m) of every comparison of the GPU test through the bars besides PAIRS x HEADS x MULTS on std1."""
    out = [(c, sq, n, pad_min(n), h, m) for c in CLASSES for sq, n, h, m in CLASS_SHAPES]
    out += [(c, sq, n, pad_min(n), h, float(m)) for c, sq, n, h, m in K2_CASES + PRODUCT_CASES]
    return out + [("std1", sq, n, n_pad, h, 472.0) for sq, n, n_pad, h in MEM_PROBS]


def table_cases():
    """(n_keys, n_pad, n_out, heads): the full product of the key cases, N_OUT and HEADS (240 tiny launches)."""
    return [(n, n_pad, n_out, heads) for n, n_pad in KEY_CASES for n_out in N_OUT for heads in HEADS]


# ---------------------------------------------------------------------------------------------------------------------
# the data classes
def _seed(name, *dims):
    s = sum(map(ord, name))
    for d in dims:
        s = s * 1009 + int(d)
    return s % (2 ** 31)


def probs_inputs(name, sq, n, heads):
    """bf16 (q [sq, H*128], k [n, H*128]) and the softmax scale of one class:
    std1 / std3 / std8   normal data, logit standard deviation 1 / 3 / 8;
    pad_dominant         q = 1 + 0.3 N, the last key 0.25 + 0.3 N, the others 0.3 N: with m = 472 the last key holds > 0.9 of every row
                         (asserted by `case`); the production-like class — the prompt's padding carries the row;
    pad_negligible       the same with the last key at -2 + 0.3 N: its weight is below 2^-20 at any m <= 511 (asserted), the residue tiny;
    far_below / _above   every score about 200 log2 units below / above zero (attention_fwd_refs' classes): the softmax is invariant
                         under the shift, a wrong maximum or a masked column taken for a key is not;
    uniform              k = 0 (m = 1, n a power of two): every weight exactly 1 / n, the residue exactly 0;
    one_hot              k_j = 64 e_j and q_row = 64 e_{j(row)} per head, j(row) = (row + head) mod n: the hot score is 4096 scale log2 e
                         = 522 log2 units above every other (raw score 4096, whose product with c is exact), so every other weight is
                         exactly 0 and the hot one exactly 1, on the last key and off it (the residue of a hot last key at m != 1:
                         `one_hot_report`)."""
    g = torch.Generator().manual_seed(_seed(name, sq, n, heads))
    D = heads * HD
    q, k = torch.randn((sq, D), generator=g), torch.randn((n, D), generator=g)
    scale = 1.0 / math.sqrt(HD)
    if name in ("std1", "std3", "std8"):
        a = math.sqrt(float(name[3:]))
        q, k = q * a, k * a
    elif name in ("pad_dominant", "pad_negligible"):
        q, k = 1.0 + 0.3 * q, 0.3 * k
        k[n - 1] += 0.25 if name == "pad_dominant" else -2.0
    elif name in ("far_below", "far_above"):
        q, k = 3.5 + 0.1 * q, (-3.5 if name == "far_below" else 3.5) + 0.1 * k
    elif name == "uniform":
        k = torch.zeros_like(k)
    elif name == "one_hot":
        q, k = torch.zeros_like(q), torch.zeros_like(k)
        for h in range(heads):
            k[torch.arange(n), h * HD + torch.arange(n)] = 64.0
            q[torch.arange(sq), h * HD + hot_key(torch.arange(sq), h, n)] = 64.0
    else:
        raise ValueError(name)
    return q.to(BF), k.to(BF), scale


def hot_key(row, head, n):
    return (row + head) % n


def table_inputs(name, n, heads, n_out):
    """bf16 (v [n, H*128], w_o [n_out, H*128]):
    integers   v in -2 .. 2, w_o in -1 .. 1: every partial sum is an integer of magnitude <= 256, exact in fp32 and in bf16;
    selector   each head slice of a w_o row is one +-2^e (e in -2 .. 2) at d(row, head) = (row + 17 head) mod 128, v random bf16 bit
               patterns of gemm_refs' band: U[row, head, j] is that one element of v shifted, exact;
    gauss      v ~ N(0, 1), w_o ~ N(0, 1) / sqrt(128); below gemm_refs.SMALL outputs drawn again until the restatement gives the fp64
               chain's bits (bar (a) asks for equal bits there), as gemm_refs.gauss_inputs does."""
    D = heads * HD
    for attempt in range(256):
        g = torch.Generator().manual_seed(_seed(name, n, heads, n_out, attempt))
        if name == "integers":
            v = torch.randint(-2, 3, (n, D), generator=g).float()
            w = torch.randint(-1, 2, (n_out, D), generator=g).float()
        elif name == "selector":
            v = G._band_bf16((n, D), g).float()
            w = torch.zeros((n_out, D))
            rows = torch.arange(n_out)
            for h in range(heads):
                e = torch.randint(-2, 3, (n_out,), generator=g).float()
                sgn = torch.randint(0, 2, (n_out,), generator=g).float() * 2 - 1
                w[rows, h * HD + selector_d(rows, h)] = sgn * torch.exp2(e)
        elif name == "gauss":
            v, w = torch.randn((n, D), generator=g), torch.randn((n_out, D), generator=g) / math.sqrt(HD)
        else:
            raise ValueError(name)
        v, w = v.to(BF), w.to(BF)
        if name != "gauss" or n_out * heads * (n + 1) >= G.SMALL:
            return v, w
        n_pad = pad_min(n)
        if torch.equal(bits(table_f32(v, w, heads, n_pad)), bits(table_ref(v, w, heads, n_pad).out)):
            return v, w
    raise RuntimeError(f"table_inputs({name}, {n}, {heads}, {n_out}): no draw is clear of the rounding boundaries")


def selector_d(row, head):
    return (row + 17 * head) % HD


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 references
def _heads(t, heads):
    return t.view(t.shape[0], heads, HD).transpose(0, 1)              # [H, S, 128]


def probs_ref(q, k, heads, scale, m):
    """(p [Sq, H, n] fp64: the last column is the m copies' total; S_abs [Sq, H, n] = sum_d |q_d k_d|, unscaled)."""
    Q, K = _heads(q.double(), heads), _heads(k.double(), heads)
    s = scale * (Q @ K.transpose(1, 2))
    s[:, :, -1] += math.log(m)
    return torch.softmax(s, -1).transpose(0, 1).contiguous(), (Q.abs() @ K.abs().transpose(1, 2)).transpose(0, 1).contiguous()


def probs_layout(p, n_pad):
    """The documented image of p [Sq, H, n] -> bf16 [Sq, H, n_pad]."""
    sq, heads, n = p.shape
    out = torch.zeros((sq, heads, n_pad), dtype=torch.float64)
    out[:, :, :n] = rb(p)
    out[:, :, n] = rb(p[:, :, -1] - rb(p[:, :, -1]))
    return out.to(BF)


def _table_layout(t, n_pad):
    """[N, H, n] -> [N, H*n_pad]: column n a copy of column n - 1, zeros after it."""
    N, heads, n = t.shape
    out = torch.zeros((N, heads, n_pad), dtype=t.dtype)
    out[:, :, :n] = t
    out[:, :, n] = t[:, :, -1]
    return out.view(N, heads * n_pad)


def table_sums(v, w_o, heads):
    """(acc, S) [N, H, n] fp64: sum_d v w_o and sum_d |v w_o|."""
    V, W = _heads(v.double(), heads), _heads(w_o.double(), heads)
    return (W @ V.transpose(1, 2)).transpose(0, 1).contiguous(), (W.abs() @ V.abs().transpose(1, 2)).transpose(0, 1).contiguous()


def table_ref(v, w_o, heads, n_pad):
    """gemm_refs.Ref of U [N, H*n_pad]: one bf16 rounding of the fp64 sum, S = sum_d |v w_o| (K = 128 for judge)."""
    acc, S = table_sums(v, w_o, heads)
    return G.Ref(*G.chain(_table_layout(acc, n_pad), None, G.EPI_BIAS, None, None, None, _table_layout(S, n_pad)), None, None)


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 restatements, with the faults
def _natural_groups():
    """src[pos] for the fault d_groups_natural: inside 32 keys, lane half h element 4 g + i taken for key 16 h + 4 g + i where the
    MFMA's D fragment holds key 8 g + 4 h + i."""
    src = torch.arange(MAXK)
    for base in (0, 32):
        for h in range(2):
            for g4 in range(4):
                for i in range(4):
                    src[base + 16 * h + 4 * g4 + i] = base + 8 * g4 + 4 * h + i
    return src


def probs_f32(q, k, heads, scale, m, n_pad, fault=None):
    """bf16 [Sq, H, n_pad] of gf_cross_probs restated.  Faults:
    residue_dropped       column n stays 0;                     residue_shifted      the residue lands in column n + 1;
    mult_missing          no multiplicity bias;                 mult_on_wrong_key    the bias on key n - 2;
    mask_drops_last       key n - 1 masked;                     mask_reads_one_past  the zero key n takes part in the softmax;
    halves_swapped        keys j and j ^ 32 exchanged (n > 32); d_groups_natural     the D fragment's 4-key groups in natural order;
    max_first_half        the maximum over keys < 32 only;      norm_by_rounded_sum  the row sum of the bf16-rounded weights;
    head_plus_one         head h reads k of head h + 1;         row_2pct             query row Sq / 2 of head 0 is 2 % too large."""
    assert fault is None or fault in PROBS_FAULTS, fault
    sq, n = q.shape[0], k.shape[0]
    c = np.float32(A.factor(scale))
    bias = 0.0 if m == 1 else float(np.float32(np.log2(np.float32(m))) / c)
    Q, K = _heads(q.float(), heads), _heads(k.float(), heads)
    out = torch.zeros((sq, heads, MAXK), dtype=BF)
    for h in range(heads):
        s = torch.full((sq, MAXK), -math.inf, dtype=torch.float32)
        s[:, :n] = Q[h] @ K[(h + 1) % heads if fault == "head_plus_one" else h].T
        if fault == "mask_drops_last":
            s[:, n - 1] = -math.inf
        if fault == "mask_reads_one_past":
            s[:, n] = 0.0
        if fault != "mult_missing":
            s[:, max(n - (2 if fault == "mult_on_wrong_key" else 1), 0)] += bias
        mx = (s[:, :32] if fault == "max_first_half" else s).max(1).values
        mc = (mx.double() * float(c)).float()
        t = (s.double() * float(c) - mc.double()[:, None]).float()                 # one rounding: the fma
        e = torch.exp2(t)
        l = (e.to(BF).float() if fault == "norm_by_rounded_sum" else e).sum(1)
        inv = 1.0 / l
        w = e * inv[:, None]
        if fault == "row_2pct" and h == 0:
            w[sq // 2] *= 1.02
            e = e.clone()
            e[sq // 2] *= 1.02
        # the residue as the compiler contracts `wl - bf16(wl)`, wl = pl * inv: fma(pl, inv, -bf16(wl)), the EXACT product less the rounded weight
        lo = (e[:, n - 1].double() * inv.double() - w[:, n - 1].to(BF).double()).float().to(BF)
        o = w.to(BF)
        if fault == "residue_shifted":
            if n + 1 < MAXK:
                o[:, n + 1] = lo
        elif fault != "residue_dropped":
            o[:, n] = lo
        if fault == "halves_swapped" and n > 32:
            o = o[:, torch.arange(MAXK) ^ 32]
        if fault == "d_groups_natural":
            o = o[:, _natural_groups()]
        out[:, h] = o
    return out[:, :, :n_pad].contiguous()


def table_f32(v, w_o, heads, n_pad, fault=None):
    """bf16 [N, H*n_pad] of gf_cross_fold_table restated: acc = fma(v_d, w_d, acc) for d = 0 .. 127 (the product of two bf16 values and
    its sum with an fp32 are exact in fp64, so the rounding to fp32 is the fma's one rounding).  Faults:
    table_col_zero            column n is zero;             table_col_from_n_minus_2   column n copies column n - 2;
    table_bf16_partials       the sum is rounded to bf16 after every 32 terms;
    table_head_slice_off      head h multiplies with w_o's slice of head h + 1."""
    assert fault is None or fault in TABLE_FAULTS, fault
    V, W = _heads(v.double(), heads), _heads(w_o.double(), heads)
    if fault == "table_head_slice_off":
        W = W[[(h + 1) % heads for h in range(heads)]]
    acc = torch.zeros((heads, w_o.shape[0], v.shape[0]), dtype=torch.float32)
    for d in range(HD):
        acc = (acc.double() + W[:, :, d, None] * V[:, None, :, d]).float()
        if fault == "table_bf16_partials" and d % 32 == 31:
            acc = rb(acc)
    n = v.shape[0]
    out = _table_layout(acc.transpose(0, 1).contiguous(), n_pad).to(BF).view(-1, heads, n_pad)
    if fault == "table_col_zero":
        out[:, :, n] = 0
    if fault == "table_col_from_n_minus_2":
        out[:, :, n] = out[:, :, max(n - 2, 0)]
    return out.view(-1, heads * n_pad)


# ---------------------------------------------------------------------------------------------------------------------
# the bounds of P
def rel_error(S_abs, scale, m):
    """E [Sq, H, n]: the docstring's derivation."""
    c = A.factor(scale)
    B = math.log2(m)
    cS = c * S_abs
    cS_max = cS.amax(-1, keepdim=True)
    d = 128 * 2 * EPS * cS + 3 * EPS * cS + EPS * (cS + cS_max + B)
    d[:, :, -1] += EPS * (cS[:, :, -1] + B) + 4 * EPS * B
    total = LN2 * (d + d.amax(-1, keepdim=True)) + 2 * 2 * EPS + 64 * EPS + 2 * EPS + EPS
    return (1 + U8) * torch.expm1(total)


def case(name, sq, n, n_pad, heads, m):
    """One case: inputs, the fp64 reference and the per-element bounds, computed once (callers cache it and leave it unchanged)."""
    q, k, scale = probs_inputs(name, sq, n, heads)
    p, S_abs = probs_ref(q, k, heads, scale, m)
    E = rel_error(S_abs, scale, m)
    if name == "pad_dominant":
        assert float(p[:, :, -1].min()) > 0.9, float(p[:, :, -1].min())
    if name == "pad_negligible":
        assert float(p[:, :, -1].max()) < 2.0 ** -20, float(p[:, :, -1].max())
    elem = U8 * p + p * E + FLOOR
    last = U16 * p[:, :, -1] + p[:, :, -1] * E[:, :, -1] + FLOOR
    row = elem[:, :, :-1].sum(-1) + last
    return types.SimpleNamespace(name=name, q=q, k=k, scale=scale, m=m, heads=heads, n=n, n_pad=n_pad, p=p, S_abs=S_abs, E=E,
                                 elem=elem, last=last, row=row, want_bits=bits(rb(p)), _f32=None)


def restated(cs):
    """probs_f32 of a case, computed once."""
    if cs._f32 is None:
        cs._f32 = probs_f32(cs.q, cs.k, cs.heads, cs.scale, cs.m, cs.n_pad)
    return cs._f32


def differing(got, cs):
    return int((bits(got[:, :, :cs.n]) != cs.want_bits).sum())


def _worst(err, allow):
    r = torch.where(allow > 0, err / allow, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(torch.nan_to_num(r, nan=math.inf, posinf=math.inf).max())


@functools.lru_cache(maxsize=None)
def bits_cap(n, p, tail=G.TAIL):
    """gemm_refs.cap's quantity — the smallest c with P[Binomial(n, p) > c] < tail — where n p is large.  gemm_refs.cap sums the upper
    tail from c + 1 on and stops at the first term below 1e-30, which is right for the means it was written for (n p of a few) and
    returns 0 once P[X = 1] itself is below 1e-30 (n p above ~80: far_below at 8 heads has 64 000 elements at a rate of 1.3e-3).  Below
    a mean of 30 this IS gemm_refs.cap; above it the same tail is summed over the whole support (log-gamma terms, fp64)."""
    if n * p < 30:
        return G.cap(n, p, tail)
    i = torch.arange(0, n + 1, dtype=torch.float64)
    logpmf = (math.lgamma(n + 1) - torch.lgamma(i + 1) - torch.lgamma(n - i + 1) + i * math.log(p) + (n - i) * math.log1p(-p))
    upper = torch.flip(torch.cumsum(torch.flip(torch.exp(logpmf), [0]), 0), [0])           # upper[c] = P[X >= c]
    return int(torch.nonzero(upper[1:] < tail)[0])                                         # the smallest c with P[X >= c + 1] < tail


def judge_probs(got, cs):
    """-> dict of the five bars' figures for got [Sq, H, n_pad] bf16: worst ratios `elem`, `last`, `row`; `zeros` (bool); `differing`
    with `cap`, `rate` (the restatement's share on the same inputs, the count taken as at least 1) and `share`."""
    assert got.shape == (cs.p.shape[0], cs.heads, cs.n_pad) and got.dtype == BF, (got.shape, got.dtype)
    n, g = cs.n, got.double()
    numel = cs.p.numel()
    rate = max(differing(restated(cs), cs), 1) / numel
    d = differing(got, cs)
    tail = got[:, :, n + 1:].contiguous().view(torch.int16)
    return dict(elem=_worst((g[:, :, :n] - cs.p).abs(), cs.elem), last=_worst((g[:, :, n - 1] + g[:, :, n] - cs.p[:, :, -1]).abs(), cs.last),
                row=_worst((g[:, :, :n + 1].sum(-1) - 1).abs(), cs.row), zeros=bool((tail == 0).all()), differing=d, share=d / numel,
                rate=rate, cap=numel if 2 * rate >= 1 else bits_cap(numel, 2 * rate), numel=numel)


BARS = ("elem", "last", "row", "zeros", "bits")


def failed_bars(j):
    """The names of the bars a judge_probs() result is outside."""
    out = [b for b in ("elem", "last", "row") if not j[b] <= 1.0]
    if not j["zeros"]:
        out.append("zeros")
    if j["differing"] > j["cap"]:
        out.append("bits")
    return out


def describe_probs(j):
    return (f"element {j['elem']:.3f}, last key + residue {j['last']:.3f}, row sum {j['row']:.3f} of their allowances; differing bits "
            f"{j['differing']}/{j['numel']} = {j['share']:.2e} (restatement {j['rate']:.2e}, cap {j['cap']}); pad columns "
            f"{'zero' if j['zeros'] else 'NOT ZERO'}")


def assert_probs(got, cs, what):
    j = judge_probs(got, cs)
    print(f"PROBS {what}: {describe_probs(j)}")
    bad = failed_bars(j)
    assert not bad, f"{what}: outside {bad}: {describe_probs(j)}"
    return j


def old_probs_bars(got, cs):
    """The bars tests/test_cross_fold_gpu.py::test_cross_probs_vs_fp64_softmax held before: True if `got` passes them."""
    n, g = cs.n, got.double()
    ok = torch.equal(got[:, :, n + 1:], torch.zeros_like(got[:, :, n + 1:]))
    ok = ok and bool(((g[:, :, :n] - cs.p).abs() <= cs.p * (2.0 ** -8 + 1e-4) + 1e-7).all())
    ok = ok and bool(((g[:, :, n - 1] + g[:, :, n] - cs.p[:, :, -1]).abs() <= cs.p[:, :, -1] * 2e-4 + 1e-7).all())
    return ok and float((g.sum(-1) - 1).abs().max()) < 2e-2


def one_hot_report(got, cs):
    """None if got is the exact one-hot image, else a message naming row, head, expected and found column.  One place is not exact, and
    the first form of this class ("the residue is 0 for any m") was wrong about it: where the hot key is the LAST key and m != 1, its
    score 4096 + log2f(m) / c is no power of two, fl(max c) is rounded, the fma returns that rounding's remainder r != 0, exp2(r) is
    1 + a few ulps, and the row sum's reciprocal is rounded: w = e fl(1 / e) is 1 to within 1.5 x 2^-23 and bf16(w) is 1.0 exactly, but
    the residue column holds w - 1 (the device: -3.8e-10, the contracted fma's exact product less 1).  There |residue| <= 2^-22 is asked
    (one ulp of the reciprocal, the product's rounding, the residue's own); everywhere else every bit."""
    want = probs_layout(cs.p, cs.n_pad)
    sq = got.shape[0]
    loose = torch.zeros(got.shape, dtype=torch.bool)
    if cs.m != 1:
        hot_last = hot_key(torch.arange(sq)[:, None], torch.arange(cs.heads)[None, :], cs.n) == cs.n - 1
        loose[:, :, cs.n] = hot_last
    bad = ((got.view(torch.int16) != want.view(torch.int16)) & ~loose) | (loose & ~(got.float().abs() <= 2.0 ** -22))
    if not bool(bad.any()):
        return None
    row, head = (int(x) for x in torch.nonzero(bad.any(-1))[0])
    found = torch.nonzero((got[row, head].float() != 0) | got[row, head].float().isnan()).flatten().tolist()
    return (f"one_hot n_keys {cs.n} m {cs.m}: row {row} head {head}: expected 1.0 in column {int(hot_key(row, head, cs.n))} and zeros elsewhere, "
            f"found non-zero columns {found} = {got[row, head][found].float().tolist()}")


# ---------------------------------------------------------------------------------------------------------------------
# the folded product
def product_ref(cs, v, w_o, b):
    """(F [Sq, N] fp64: sum_h P_h V_h W_o,h^T + b, the per-element bound of the docstring) for a probs case and its table operands."""
    acc, S = table_sums(v, w_o, cs.heads)                              # [N, H, n]
    F = torch.einsum("shj,nhj->sn", cs.p, acc) + b.double()
    Ua = acc.abs()
    pP = cs.p * (U8 + cs.E)
    pP[:, :, -1] = cs.p[:, :, -1] * (U16 + cs.E[:, :, -1])
    bound = torch.einsum("shj,nhj->sn", pP, Ua) + torch.einsum("shj,nhj->sn", cs.p * (1 + U8 + cs.E), U8 * Ua + 128 * 2 * EPS * S)
    return F, bound + FLOOR * Ua.sum((1, 2))


def product_hat(p_hat, u_hat, b):
    """P^ U^^T + b in fp64 from [Sq, H*n_pad] and [N, H*n_pad] bf16."""
    return p_hat.double() @ u_hat.double().T + b.double()


def unfolded_chain(cs, v, w_o, b):
    """The unfolded path's bf16 chain in fp64 with its roundings: O = bf16(P V) per head, then bf16(O W_o^T + b)."""
    V = _heads(v.double(), cs.heads)                                   # [H, n, 128]
    O = rb(torch.einsum("shj,hjd->shd", cs.p, V)).reshape(cs.p.shape[0], -1)
    return rb(O @ w_o.double().T + b.double())
