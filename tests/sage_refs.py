"""Hand-built operands, the recipe, an fp32 restatement and the bars of the SageAttention kernels (goal_force_amd/csrc/
gf_sage_attention.hip; the contract: include/goalforce.h).  Plain helper: CPU tensors in, CPU tensors out, no GPU, no project import.

An `Ops` holds what gf_sage_attn_fwd takes, in the header's layouts: q8 [q_len, H*128] int8, qs [H, ceil(q_len / 32)], k8 [kv_pad8, H*128]
int8, ks [H, kv_pad8 / 64], vt8 [H*128, kv_pad8] e4m3 codes (key k of a 128-key slice at sage_oracle.vt_position), vs [H, 128].

`recipe(op)` walks the header's recipe once and returns a `Ref`:
  out    the fp64 recipe on exact sums, before its one rounding: fp32 w = fp32(fp32(s_q s_k) c), fp32 row maximum of fp32(dot w), the one
         fp32 FMA x = fp32(dot w + fp32(8 - m)), P = e4m3(fp32(exp2 x)), l = sum P, acc = sum P V_code, alpha = exp2(m_old - m_new),
         O = acc / l * v_scale — sage_oracle.attention on given codes;
  model  the same with the sums of every 128-key tile formed by gemm_refs.mfma_fp8 (the measured model of the f8f6f4 MFMA, keys in the
         order of their V^T positions, the row sum as a 129th channel of e4m3 1.0), rounded to bf16: what bar (a) compares bits with;
  bound  bar (b), below;  excused  [q_len, H] bool: the pairs that hold an ambiguous P;  acc, l  the exact sums (fp64, code units).
`restate(op, fault=None)` is the kernel's path in fp32 from the header alone (fp32 alpha = fp32(exp2(fp32(m_old - m_new))), fp32
accumulators that take every tile's mfma_fp8 sum with one rounding, and `tail`): tests/test_sage_refs_cpu.py shows that it passes the
exact classes with equality and both bars on every gauss input of the GPU test, and that each of FAULTS does not.

The exact classes (builders `one_hot`, `uniform`, `staircase`; the softmax scale fp32(ln 2 2^-k) makes the launcher's factor exactly
2^-k, `pow2_scale`) have power-of-two w, integer exp2 arguments and P an exact power of two or 0; their expectation is
    tail(acc, l, v_scale) = bf16(fp32(fp32(acc fp32(1 / l)) v_scale))
of the recipe's exact sums, which are fp32 values (`exact_tail`; `one_hot`: the hot key's V code times v_scale).  The CPU test shows
`restate` equal to it: nothing rounds before the tail.  (bf16 of the fp64 quotient is NOT the expectation: the tail's three fp32
roundings move 1 staircase element in 66 048 across a bf16 boundary.)  They rest on the device's exp2 being exact at integer arguments
(measured: it is, profiles/r20).

The two bars of the gauss class (`judge`):
  (a) the share of bf16 bits differing from `model` over the pairs that are not excused is at most gemm_refs.SHARE_CAP = 2^-10 (where
      2^-10 numel < 1 the bits are equal), and the count in every (row, head) (128 elements) and every column (head, channel) is at
      most cross_fold_refs.bits_cap(n, 2^-10).  A P whose fp64 value lies within a relative 2^-21 of an e4m3 rounding boundary (the
      midpoints of neighbouring e4m3 values, the subnormal steps k 2^-9 and the underflow tie 2^-10 included) is AMBIGUOUS: one fp32
      ulp of exp2 (2^-23 relative; 2^-21 leaves a factor 4) may round it either way.  A (row, head) holding one is excused from (a)
      and judged by (b) alone; at most 2 % of the pairs may be excused (asserted: a condition, not a measurement).
  (b) every element: |got - out| <= the sum of
        2^-8 |out|                                               the one bf16 rounding (the convention of attention_fwd_refs: a value
                                                                 moved by the other terms may round to the far neighbour);
        sum over ambiguous P_j: step(P_j) a_j |V_j - O| s_v / l  one e4m3 step of P_j (2^-3 of its binade, 2^-9 below 2^-6), a_j =
                                                                 exp2(m at j's tile - final m), O = acc / l in code units: the move of
                                                                 acc_j and of l together;
        (T_acc + T_l |O|) s_v / l                                mfma_fp8's truncation bound T, carried through the later alphas; on l
                                                                 through the quotient;
        17 nt 2^-23 (S / l + |O|) s_v                            the fp32 accumulation: per tile 16 group sums and the add onto the
                                                                 accumulator, each within one fp32 ulp of a partial sum <= S = sum P |V|
                                                                 (for l: <= l);
        2 n_moved 2^-23 (S / l + |O|) s_v                        the alpha products: one fp32 rounding and one ulp of exp2 per tile at
                                                                 which the maximum moved, on what was accumulated before;
        2^-22 |out|                                              the tail: fp32(1 / l) and its two multiplies, 2^-24 each.
      Non-finite `got` is outside.  Nothing here is fitted to the kernel.
"""
import collections
import math

import numpy as np
import torch

import cross_fold_refs as CF
import gemm_refs as G
import sage_oracle as so

BF = torch.bfloat16
E4M3 = torch.float8_e4m3fn
HD, T, E = 128, 128, 8.0
INT_MIN = -2.0 ** 31
FLT_MAX = float(np.finfo(np.float32).max)
AMBIG = 2.0 ** -21
EXCUSED_CAP = 0.02
ULP32 = 2.0 ** -23
FINITE = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)          # every finite e4m3 code, both signs
Q_LENS = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 257)
KV_LENS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 385, 513)
UNIFORM_KV = tuple(range(1, 131)) + (191, 192, 193, 255, 256, 257, 385, 513)
HEADS = (1, 3, 5)
VT_KV = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193, 257)
MEAN_ROWS = (1, 2, 63, 64, 65, 127, 129, 4097)
# (q_len, kv_len, heads, shift) of one_hot: every kv_len edge (whole and ragged last tiles and 64-key halves, the 4-key lane group and
# the 16-key block) and every q_len edge at least once
ONE_HOT_CASES = ((257, 513, 3, 0), (129, 385, 5, 0), (1, 129, 1, 5), (15, 97, 3, 64), (17, 65, 1, 100), (33, 193, 3, 90), (31, 257, 5, 0),
                 (127, 191, 3, 0), (128, 255, 1, 0), (16, 4, 1, 3), (32, 1, 3, 0), (33, 3, 1, 7), (17, 5, 3, 0), (32, 15, 1, 20), (129, 16, 3, 0),
                 (31, 17, 1, 50), (129, 63, 3, 0), (129, 64, 3, 0), (257, 127, 1, 0), (129, 128, 3, 0), (129, 192, 3, 0), (257, 256, 5, 0))
FAULTS = ("drop_last_key", "one_past", "intmin_only", "keep_only", "no_hvalid", "vt_natural", "k_scale_next", "q_scale_next",
          "l_unquantised", "rescale_skips_l", "alpha_one_qb", "v_scale_next_head", "row_2pct")

Ops = collections.namedtuple("Ops", "q8 qs k8 ks vt8 vs q_len kv_len heads scale")
Ref = collections.namedtuple("Ref", "out model bound excused acc l")


def pad128(n):
    return -(-n // T) * T


def pow2_scale(k):
    """The softmax scale fp32(ln 2 2^-k): the launcher's fp32(scale x 1.4426950408889634f) is exactly 2^-k (k = 0 .. 7)."""
    s = float(np.float32(math.log(2.0) * 2.0 ** -k))
    assert so.softmax_factor(s) == 2.0 ** -k, k
    return s


def e4m3_codes(x):
    """fp32 / fp64 values -> e4m3fn codes (uint8), round to nearest even."""
    return x.float().to(E4M3).view(torch.uint8)


def decode(c):
    return c.view(E4M3).float().double()


def tail(acc, l, vs):
    """bf16(fp32(fp32(acc fp32(1 / l)) v_scale)) of fp32 tensors acc [R, 128], l [R], vs [128]."""
    assert acc.dtype == l.dtype == vs.dtype == torch.float32
    return ((acc * (1.0 / l)[:, None]) * vs[None, :]).to(BF)


def empty_ops(q_len, kv_len, heads, k):
    kvp = pad128(kv_len)
    return Ops(torch.zeros((q_len, heads * HD), dtype=torch.int8), torch.ones((heads, -(-q_len // 32))),
               torch.zeros((kvp, heads * HD), dtype=torch.int8), torch.ones((heads, kvp // 64)),
               torch.zeros((heads * HD, kvp), dtype=torch.uint8), torch.ones((heads, HD)), q_len, kv_len, heads, pow2_scale(k))


def place_v(op, codes):
    """codes [kv_len, H, 128] uint8 -> op.vt8 at sage_oracle.vt_position; pad positions keep code 0."""
    pos = so.vt_position(op.kv_len)
    op.vt8.view(op.heads, HD, -1)[:, :, pos] = codes.permute(1, 2, 0)


def v_codes(op):
    """-> [kv_len, H, 128] codes read back through vt_position."""
    return op.vt8.view(op.heads, HD, -1)[:, :, so.vt_position(op.kv_len)].permute(2, 0, 1)


# ---------------------------------------------------------------------------------------------------------------------
# the exact classes
def hot_keys(kv_len, heads, where):
    """[H, 128]: the hot key of every (head, channel).  where = 'first' / 'last': all in that tile; 'spread': heads cycle through the
    first, middle and last tile.  Inside the tile the 128 channels walk every key of it (a stride coprime to its length), channel 0
    takes the tile's last valid key; from 129 keys on channels 1 .. 4 of head 0 take keys 63, 64, 127, 128."""
    nt = -(-kv_len // T)
    hot = torch.zeros((heads, HD), dtype=torch.long)
    for h in range(heads):
        t = dict(first=0, last=nt - 1, spread=(0, nt // 2, nt - 1)[h % 3])[where]
        n = min(kv_len, T * t + T) - T * t
        step = next(s for s in (37, 5, 3, 1) if math.gcd(s, n) == 1)
        hot[h] = T * t + (n - 1 + step * torch.arange(HD) + h) % n
        hot[h, 0] = T * t + n - 1
    if kv_len > 128 and where == "spread":
        hot[0, 1:5] = torch.tensor([63, 64, 127, 128])
    return hot


def one_hot(q_len, kv_len, heads, where="spread", shift=0):
    """q8[row] = 127 e_c, c = (row + shift) mod 128; k8[j][c] = 127 at the hot key of c, else -127; s_q = 2, s_k = 1/2, c = 2^-7: the
    hot score is 16129 / 128, every other its negative, 252 log2 units below.  V[j] carries every finite e4m3 code (index j + c mod 254
    on even channels, 2 j + c mod 253 on odd ones: no two keys below 64 262 share a row); v_scale = 2^((c + h) mod 5 - 2).
    -> (op, hot [H, 128], want [q_len, H*128] bf16 = V[hot] v_scale)."""
    op = empty_ops(q_len, kv_len, heads, 7)
    op.qs.fill_(2.0)
    op.ks.fill_(0.5)
    hot = hot_keys(kv_len, heads, where)
    c = (torch.arange(q_len) + shift) % HD
    q3, k3 = op.q8.view(q_len, heads, HD), op.k8.view(-1, heads, HD)
    q3[torch.arange(q_len), :, c] = 127
    k3[:kv_len] = -127
    for h in range(heads):
        k3[hot[h], h, torch.arange(HD)] = 127
    j, ch = torch.arange(kv_len)[:, None, None], torch.arange(HD)[None, None, :]
    idx = torch.where(ch % 2 == 0, (j + ch) % 254, (2 * j + ch) % 253) + 0 * torch.arange(heads)[None, :, None]
    place_v(op, FINITE[idx])
    op.vs.copy_(torch.exp2(((torch.arange(HD)[None, :] + torch.arange(heads)[:, None]) % 5 - 2).float()))
    want = decode(v_codes(op))[hot[:, c], torch.arange(heads)[:, None]].transpose(0, 1) * op.vs.double()[None]      # [q_len, H, 128]
    return op, hot, want.reshape(q_len, -1).to(BF)


def one_hot_report(got, op, hot, want, shift=0):
    """None, or a message naming the first wrong (row, head), the expected key and the key whose V row was found there."""
    bad = torch.nonzero((got.float() != want.float()).view(op.q_len, op.heads, HD).any(-1))
    if not len(bad):
        return None
    row, h = (int(x) for x in bad[0])
    rows = decode(v_codes(op))[:, h] * op.vs.double()[h]
    found = torch.nonzero((rows.to(BF).float() == got.view(op.q_len, op.heads, HD)[row, h].float()).all(-1)).flatten().tolist()
    return (f"one_hot q={op.q_len} keys={op.kv_len} heads={op.heads}: O[row {row}, head {h}] is not V[key {int(hot[h, (row + shift) % HD])}] "
            f"x v_scale; it is the row of key {found if found else 'none (a mixture)'}; {len(bad)} (row, head) pairs wrong")


def uniform(q_len, kv_len, heads, variant="q0", garbage=False):
    """Every P is 256: q8 = 0 ('q0'), q_scale = 0 ('qs0') or k_scale = 0 ('ks0') on random codes.  V codes are integers of magnitude
    1 .. 8, v_scale a power of two.  garbage: the pad rows of k8 and the pad positions of vt8 hold finite garbage and the k_scale of an
    all-pad half is NaN (the maskings must hold without zeros in the padding).  -> (op, want)."""
    g = torch.Generator().manual_seed(1000 * kv_len + heads)
    op = empty_ops(q_len, kv_len, heads, 3)
    if variant != "q0":
        op.q8.copy_(torch.randint(-127, 128, op.q8.shape, generator=g))
        op.k8[:kv_len] = torch.randint(-127, 128, (kv_len, heads * HD), generator=g).to(torch.int8)
        (op.qs if variant == "qs0" else op.ks).zero_()
        (op.ks if variant == "qs0" else op.qs).fill_(0.25)
    v = torch.randint(1, 9, (kv_len, heads, HD), generator=g) * (2 * torch.randint(0, 2, (kv_len, heads, HD), generator=g) - 1)
    if garbage:
        op.k8[kv_len:] = torch.randint(-127, 128, (op.k8.shape[0] - kv_len, heads * HD), generator=g).to(torch.int8)
        op.vt8.copy_(FINITE[torch.randint(0, len(FINITE), op.vt8.shape, generator=g)])
        if kv_len % T and kv_len % T <= 64:
            op.ks[:, -1] = math.nan
    place_v(op, e4m3_codes(v))
    op.vs.copy_(torch.exp2(((torch.arange(HD)[None, :] + 2 * torch.arange(heads)[:, None]) % 7 - 3).float()))
    acc = (256.0 * v.sum(0)).float()                                                                 # [H, 128], exact
    want = torch.stack([tail(acc[h][None], torch.tensor([256.0 * kv_len]), op.vs[h]) for h in range(heads)], 1)
    return op, want.expand(q_len, heads, HD).reshape(q_len, -1).contiguous()


STAIRS = ((0, 1, -1, 2, 0), (0, 5, 3, 6, 1), (2, 0, 6, 1, 4), (0, 2, 4, 5, 3), (1, 4, 2, 5, 5))     # tile maxima; rises 1 .. 5, and falls


def staircase(q_len, nt, heads, kv_len=None):
    """Integer scores: row r looks at channel c = r mod 128 only (q code 16 / 2^b on a Q block with s_q = 2^b, b = block mod 3; k codes
    doubled on the odd 64-key halves, whose s_k is 1/2; c = 2^-4), the score of key j is the k code: the tile maxima follow
    STAIRS[(c + h) mod 5], every key lies 0 .. 6 below the running maximum (so P = 2^2 .. 2^8), one key of every tile at its
    maximum.  V holds integers of magnitude 1 .. 4.  -> op; the expectation is restate(op) (the CPU test shows it equal to the fp64
    recipe: every fp32 step is exact up to `tail`)."""
    kv_len = T * nt if kv_len is None else kv_len
    assert -(-kv_len // T) == nt <= 5
    g = torch.Generator().manual_seed(77 * nt + heads)
    op = empty_ops(q_len, kv_len, heads, 4)
    r = torch.arange(q_len)
    b = (r // 32) % 3
    op.qs.copy_(torch.exp2((torch.arange(op.qs.shape[1]) % 3).float())[None].expand_as(op.qs))
    op.q8.view(q_len, heads, HD)[r, :, r % HD] = (16 // 2 ** b).to(torch.int8)[:, None]
    half = torch.arange(op.k8.shape[0]) // 64
    op.ks.copy_(torch.where(torch.arange(op.ks.shape[1]) % 2 == 1, 0.5, 1.0)[None].expand_as(op.ks))
    k3 = op.k8.view(-1, heads, HD)
    for h in range(heads):
        for c in range(HD):
            top = torch.tensor(STAIRS[(c + h) % 5][:nt])
            run = torch.cummax(top, 0).values
            room = 6 - (run - top)                                                                    # how far below its tile's maximum a key may lie
            t = torch.arange(kv_len) // T
            below = torch.randint(0, 7, (kv_len,), generator=g) % (room[t] + 1)
            below[T * torch.arange(nt) + (c % min(T, kv_len - T * (nt - 1)))] = 0
            k3[:kv_len, h, c] = ((top[t] - below) * (1 + half[:kv_len] % 2)).to(torch.int8)
    v = torch.randint(1, 5, (kv_len, heads, HD), generator=g) * (2 * torch.randint(0, 2, (kv_len, heads, HD), generator=g) - 1)
    place_v(op, e4m3_codes(v))
    op.vs.copy_(torch.exp2(((torch.arange(HD)[None, :] + torch.arange(heads)[:, None]) % 3 - 1).float()))
    return op


# ---------------------------------------------------------------------------------------------------------------------
# the gauss class
def gauss_qkv(sq, skv, heads, std=1.0, seed=0, blocks=True):
    """bf16 q, k, v [S, H*128]: Gaussian, logit std `std` (q and k share it), k with test_sage_attention_gpu._qkv's channel offset, and
    (blocks) Q block 1 (or 0) and K block 1 (or 0) of every head 2^6 larger than the rest."""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * sq + skv + heads)
    w = heads * HD
    q = torch.randn((sq, w), generator=g) * math.sqrt(std)
    k = torch.randn((skv, w), generator=g) * math.sqrt(std) + 0.7 * torch.randn((1, w), generator=g)
    v = torch.randn((skv, w), generator=g) + 0.3
    if blocks:
        qb, kb = (1 if sq > 32 else 0), (1 if skv > 64 else 0)
        q[32 * qb:32 * qb + 32] *= 64.0
        k[64 * kb:64 * kb + 64] *= 64.0
    return q.to(BF), k.to(BF), v.to(BF)


def k_mean(k, heads):
    """fp32(fp64 sum / n) per (head, channel)."""
    return (k.double().sum(0) / k.shape[0]).float().view(heads, HD)


def quantise(q, k, v, heads, scale=None):
    """The Ops sage_oracle's quantisers give for bf16 q, k, v (mu = k_mean), in the header's layouts."""
    sq, skv = q.shape[0], k.shape[0]
    q8, qs = so.quant_q(q, heads)
    k8, ks = so.quant_k(k, heads, k_mean(k, heads))
    v8, vs = so.quant_v(v, heads)
    op = empty_ops(sq, skv, heads, 0)._replace(scale=HD ** -0.5 if scale is None else scale)
    op.q8.copy_(q8.transpose(0, 1).reshape(sq, -1))
    op.qs.copy_(qs)
    op.k8[:skv] = k8.transpose(0, 1).reshape(skv, -1)
    op.ks.zero_()
    op.ks[:, :ks.shape[1]] = ks
    place_v(op, v8.view(torch.uint8).transpose(0, 1))
    op.vs.copy_(vs)
    return op


assert {c[1] for c in ONE_HOT_CASES} >= set(KV_LENS) and {c[0] for c in ONE_HOT_CASES} >= set(Q_LENS)


def gauss_cases():
    """(q_len, kv_len, heads, std, blocks) of the gauss edges: every q_len and every kv_len of the issue once, heads 1 / 3 / 5, std 1 / 3;
    the enlarged blocks (which make the softmax of their rows and keys nearly one-hot) on every other case and on the three large
    shapes both ways."""
    n = max(len(Q_LENS), len(KV_LENS))
    return [(Q_LENS[(3 * i) % len(Q_LENS)], KV_LENS[i % len(KV_LENS)], HEADS[i % 3], (1.0, 3.0)[i % 2], i % 4 < 2) for i in range(n)] + \
           [(sq, skv, h, std, b) for sq, skv, h, std in ((257, 385, 3, 1.0), (129, 513, 3, 3.0), (257, 513, 5, 1.0)) for b in (False, True)]


# ---------------------------------------------------------------------------------------------------------------------
# the recipe, the model and the restatement
def _step(p):
    """The e4m3 spacing at p > 0 (fp64)."""
    return torch.exp2(torch.clamp(torch.floor(torch.log2(p.clamp_min(1e-300))), min=-6.0) - 3.0)


def ambiguous(p):
    """p (fp64, > 0, <= 256): within a relative AMBIG of a midpoint between two neighbouring e4m3 values."""
    s = _step(p)
    f = p / s
    return ((f - torch.floor(f) - 0.5).abs() * s <= AMBIG * p) & (p < 480.0)


def _walk(op, f32, fault=None):
    """One pass over the tiles of every head.  f32 = False -> Ref; f32 = True -> the restatement's O [q_len, H*128] bf16."""
    R, H, kv = op.q_len, op.heads, op.kv_len
    nt, kvp = -(-kv // T), pad128(kv)
    c = torch.tensor(so.softmax_factor(op.scale), dtype=torch.float32)
    pos = so.vt_position(T)
    rows = torch.arange(R)
    qblk = torch.clamp(rows // 32 + (1 if fault == "q_scale_next" else 0), max=op.qs.shape[1] - 1)
    outs, models, bounds, excused, accs, ls = [], [], [], [], [], []
    ones = torch.full((1, T), 0x38, dtype=torch.uint8)
    for h in range(H):
        q = op.q8.view(R, H, HD)[:, h].double()
        k = op.k8.view(kvp, H, HD)[:, h].double()
        vt = op.vt8.view(H, HD, kvp)[h]
        vs = op.vs[(h + 1) % H if fault == "v_scale_next_head" else h]
        sq = op.qs[h, qblk].float()
        m = torch.full((R,), -math.inf, dtype=torch.float32)
        dt = torch.float32 if f32 else torch.float64
        acc, l = torch.zeros((R, HD), dtype=dt), torch.zeros((R,), dtype=dt)                        # f32: the kernel's; else the model's
        xacc, xl, S = torch.zeros((R, HD), dtype=torch.float64), torch.zeros((R,), dtype=torch.float64), torch.zeros((R, HD), dtype=torch.float64)
        Tacc, Tl, moved = torch.zeros((R, HD), dtype=torch.float64), torch.zeros((R,), dtype=torch.float64), torch.zeros((R,))
        amb = []
        for t in range(nt):
            key = T * t + torch.arange(T)
            vmax, vkeep = key < kv, key < kv
            if fault == "drop_last_key":
                vmax, vkeep = key < kv - 1, key < kv - 1
            if fault == "one_past":
                vmax, vkeep = key < kv + 1, key < kv + 1
            if fault == "keep_only":
                vmax = torch.ones_like(vmax)
            if fault == "intmin_only":
                vkeep = torch.ones_like(vkeep)
            dot = q @ k[T * t:T * t + T].t()                                                          # exact integers
            sk = op.ks[h, torch.clamp(2 * t + torch.arange(T) // 64 + (1 if fault == "k_scale_next" else 0), max=op.ks.shape[1] - 1)].float()
            w = (sq[:, None] * sk[None, :]) * c                                                       # fp32(fp32(s_q s_k) c)
            hval = torch.tensor([T * t < kv, T * t + 64 < kv]).repeat_interleave(64)
            sdot = torch.where(vmax[None], dot, torch.full_like(dot, INT_MIN)).float()
            s = sdot * w                                                                              # fp32; INT_MIN x w on the masked keys
            mt = s[:, hval].amax(1)
            if fault == "no_hvalid" and not bool(hval.all()):
                mt = torch.maximum(mt, s[:, ~hval].amax(1))                                           # a NaN scale in the pad half reaches the maximum
            m_new = torch.maximum(m, mt)
            d = (m - m_new)                                                                           # fp32; -inf on the first tile
            mv = m_new > m
            alpha = torch.where(mv, torch.exp2(d.double()), torch.ones_like(d, dtype=torch.float64))
            if t:
                moved += mv
            xacc, xl, S, Tacc, Tl = xacc * alpha[:, None], xl * alpha, S * alpha[:, None], Tacc * alpha[:, None], Tl * alpha
            a = alpha.float() if f32 else alpha
            if fault == "alpha_one_qb":
                a = torch.where(rows % 32 < 16, a, torch.ones_like(a))
            acc = acc * a[:, None]
            if fault != "rescale_skips_l":
                l = l * a
            m = m_new
            off = (E - m).float()
            x = (sdot.double() * w.double() + off.double()[:, None]).float()                          # the one FMA
            p64 = torch.exp2(x.double())
            p8 = e4m3_codes(p64.float())
            p8 = torch.where(vkeep[None], p8, torch.zeros_like(p8))
            ppos = torch.zeros_like(p8)
            if fault == "vt_natural":
                ppos = p8
            else:
                ppos[:, pos] = p8
            vtile = vt[:, T * t:T * t + T]
            ms, mT = G.mfma_fp8(ppos, torch.cat([vtile, ones]))
            if fault == "l_unquantised":
                ms[:, HD] = torch.where(vkeep[None], p64, torch.zeros_like(p64)).sum(1)
            if f32:
                acc, l = (acc.double() + ms[:, :HD]).float(), (l.double() + ms[:, HD]).float()
                continue
            acc, l = acc + ms[:, :HD], l + ms[:, HD]
            P, V = decode(ppos), decode(vtile)
            xacc, xl, S = xacc + P @ V.t(), xl + P.sum(1), S + P @ V.abs().t()
            Tacc, Tl = Tacc + mT[:, :HD], Tl + mT[:, HD]
            am = ambiguous(p64) & vkeep[None] & torch.isfinite(p64)
            if bool(am.any()):
                r_, j_ = torch.nonzero(am, as_tuple=True)
                amb.append((r_, T * t + pos[j_], _step(p64[r_, j_]), m[r_].double()))
        if f32:
            o = tail(acc, l, vs)
            if fault == "row_2pct":
                o[R // 2] = (o[R // 2].float() * 1.02).to(BF)
            outs.append(o)
            continue
        vs64 = vs.double()
        oc = xacc / xl[:, None]
        out = oc * vs64[None]
        t2 = torch.zeros((R, HD), dtype=torch.float64)
        ex = torch.zeros((R,), dtype=torch.bool)
        for r_, p_, st, mt_ in amb:
            f = st * torch.exp2(mt_ - m[r_].double())
            t2.index_add_(0, r_, f[:, None] * (decode(vt[:, p_]).t() - oc[r_]).abs())
            ex[r_] = True
        sl = S / xl[:, None] + oc.abs()
        bound = (2.0 ** -8 + 2.0 ** -22) * out.abs() + (t2 / xl[:, None] + (Tacc + Tl[:, None] * oc.abs()) / xl[:, None]
                                                        + (17 * nt + 2 * moved.double()[:, None]) * ULP32 * sl) * vs64[None]
        outs.append(out)
        models.append((acc / l[:, None] * vs64[None]).to(BF))
        bounds.append(bound)
        excused.append(ex)
        accs.append(xacc)
        ls.append(xl)
    cat = lambda ts: torch.stack(ts, 1).reshape(R, H * HD)                                            # noqa: E731
    return cat(outs) if f32 else Ref(cat(outs), cat(models), cat(bounds), torch.stack(excused, 1), cat(accs), torch.stack(ls, 1))


def exact_tail(op, ref):
    """`tail` of the recipe's exact sums, which must be fp32 values (an exact class): what a kernel whose fp32 steps are all exact writes."""
    assert torch.equal(ref.acc.float().double(), ref.acc) and torch.equal(ref.l.float().double(), ref.l), "the exact sums are not fp32 values"
    a = ref.acc.float().view(op.q_len, op.heads, HD)
    return torch.stack([tail(a[:, h], ref.l[:, h].float(), op.vs[h]) for h in range(op.heads)], 1).reshape(op.q_len, -1)


def recipe(op):
    return _walk(op, False)


def restate(op, fault=None):
    return _walk(op, True, fault)


# ---------------------------------------------------------------------------------------------------------------------
# the bars
def judge(got, ref, rate=G.SHARE_CAP):
    """-> dict of both bars' figures for got [q_len, H*128] bf16."""
    R, H = ref.excused.shape
    live = ~ref.excused                                                                               # [R, H]
    diff = (G.bits(got) != G.bits(ref.model)).view(R, H, HD) & live[:, :, None]
    n = int(live.sum()) * HD
    rows_live = live.sum(0)                                                                           # per head
    col_cap = torch.tensor([CF.bits_cap(int(x), rate) if int(x) else 0 for x in rows_live])
    err = (got.double() - ref.out).abs()
    ratio = torch.where(ref.bound > 0, err / ref.bound, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    return dict(numel=n, differing=int(diff.sum()), share=int(diff.sum()) / max(n, 1), rate=rate, pair_worst=int(diff.sum(2).max()),
                pair_cap=CF.bits_cap(HD, rate), col_over=int((diff.sum(0) > col_cap[:, None]).sum()), col_worst=int(diff.sum(0).max()),
                col_cap=int(col_cap.max()), worst=float(ratio.max()), outside=int((ratio > 1).sum()), excused=float(ref.excused.double().mean()),
                first=torch.nonzero((ratio > 1).view(R, H, HD) | diff)[:3].tolist())


def failed_bars(j):
    out = []
    share_ok = j["differing"] == 0 if j["rate"] * j["numel"] < 1 else j["share"] <= j["rate"]
    if not (share_ok and j["pair_worst"] <= j["pair_cap"] and j["col_over"] == 0):
        out.append("a")
    if j["outside"]:
        out.append("b")
    if j["excused"] > EXCUSED_CAP:
        out.append("excused")
    return out


def describe(j):
    return (f"differing bits {j['differing']}/{j['numel']} = {j['share']:.2e} (cap {j['rate']:.2e}), worst (row, head) {j['pair_worst']} (cap "
            f"{j['pair_cap']}), worst column {j['col_worst']} (cap {j['col_cap']}, {j['col_over']} over); (b) worst {j['worst']:.3g} of the bound, "
            f"{j['outside']} outside; excused pairs {100 * j['excused']:.2f} %")


def assert_pinned(got, ref, what, rate=G.SHARE_CAP):
    j = judge(got, ref, rate)
    print(f"SAGE {what}: {describe(j)}")
    bad = failed_bars(j)
    assert not bad, f"{what}: outside {bad}: {describe(j)}; first (row, head, channel): {j['first']}"
    return j


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------------------------
# the quantisers
def vt32_of(v):
    """The bf16 V^T [H*128, kv_pad64] a projection would hand to gf_sage_quant_vt (vt_in = 1), built with gemm_refs.vt32_layout."""
    return G.vt32_layout(v, v.shape[0])


def quant_vt_ref(v, heads):
    """(vt8 [H*128, kv_pad8] codes at vt_position with zero padding, v_scale [H, 128]) of plain V through sage_oracle.quant_v."""
    codes, vs = so.quant_v(v, heads)
    op = empty_ops(1, v.shape[0], heads, 0)
    place_v(op, codes.view(torch.uint8).transpose(0, 1))
    return op.vt8, vs


def vt32_producer(vt32, kv_len, heads, fault=None):
    """sage_quant_vt_kernel<true> restated: the vt32 image read back to plain V (positions past kv_len ignored), then quant_vt_ref.
    fault 'halves_exchanged': keys 4 g + i and 16 + 4 g + i of every 32-key group change places."""
    p = G.vt_positions(vt32.shape[1])[:kv_len]
    if fault == "halves_exchanged":
        p = p ^ 4
    return quant_vt_ref(vt32[:, p].t().contiguous(), heads)


def exact_mean_k(rows, heads, seed=0):
    """bf16 k [rows, H*128] whose fp64 column sums are exact: magnitudes 2^-20 .. 2^6 with 8 significant bits (span 34 bits, 4097 rows
    add 13: inside fp64's 53)."""
    g = torch.Generator().manual_seed(seed + rows)
    e = torch.randint(-20, 7, (rows, heads * HD), generator=g).float()
    return ((torch.rand((rows, heads * HD), generator=g) + 1.0) * torch.exp2(e) * (2 * torch.randint(0, 2, e.shape, generator=g) - 1)).to(BF)


TINY = (2.0 ** -120, 2.0 ** -126, 2.0 ** -133)            # the last: bf16's smallest subnormal


def tiny_rows(rows, heads, amax, seed=0):
    """bf16 [rows, H*128]: +-amax, +-amax/2 (where representable) and exact zeros, every column summing to exactly zero over each pair
    of rows (so K's mean is 0 and k~ = k)."""
    assert rows % 2 == 0
    g = torch.Generator().manual_seed(seed)
    half = rows // 2
    a = torch.randint(0, 3, (half, heads * HD), generator=g).double() * (amax / 2 if amax > 2.0 ** -133 else amax)
    a = torch.where(a > amax, torch.full_like(a, amax), a)
    a[0, ::2] = amax
    x = torch.cat([a, 0.0 - a])
    return x.to(BF)
