"""The exact chain, an fp32 restatement and the two bars of the GEMM family (goal_force_amd/csrc/gf_gemm.hip: gf_gemm_bf16, gf_gemm_fp8,
gf_linear_vt32(_fp8), gf_gemm_bf16_batched).  Plain helper: CPU tensors in, CPU tensors out, no GPU and no project import.

* `product(a, w)`: (acc, S) in fp64, acc = A W^T of the operands' VALUES (bf16 values, or dequantised e4m3 codes when the operand is a
  uint8 tensor), S = |A| |W|^T.
* `chain(acc, bias, epi, resid, gate, row_scale=None, S=None)`: the epilogue as include/goalforce.h states it, all arithmetic in fp64
  with a rounding to bf16 at exactly the header's points (rs = row_scale[m] for fp8, 1 otherwise):
      EPI 0     bf16(acc rs + bias)                        EPI 3   bf16(resid + bf16(...))
      EPI 1, 4  bf16(act(bf16(...)))                       EPI 5   bf16(bf16(...) resid)
                (-0 on the header's two tail ranges, TAILS)
      EPI 2     bf16(resid + bf16(gate bf16(...)))
  It returns (chain as fp64 holding bf16 values, m, S rs, L), per element:
      m   the largest magnitude among the element's stage values and the operands of its last add or multiply
          (acc rs, bias, every rounded stage, gate's product, resid) — raised, for the epilogues with more than one rounding, to what
          a flipped FIRST rounding costs once the later stages have rounded it again (bar (b) below):
              EPI 1, 4  L |y| + |out|      EPI 2  |gate| |y| + |t| + |out|      EPI 3  |y| + |out|      EPI 5  |resid| |y| + |out|
          (y the rounded Linear, t = bf16(gate y));
      L   how far an error of the accumulator travels to the output: 1 (EPI 0, 3), |gate| (EPI 2), |resid| (EPI 5), and the largest
          slope of the activation for EPI 1 and 4:
            SiLU        f(x) = x s(x), s the logistic function: f' = s (1 + x (1 - s)), f'' = s (1 - s) (2 + x (1 - 2 s)); f'' = 0 where
                        x tanh(x / 2) = 2, x = 2.3994, s = 0.91680, f' = 0.91680 (1 + 2.3994 * 0.08320) = 1.0998  ->  L = 1.1.
            GELU-tanh   f(x) = x s(z), z = 2 sqrt(2/pi) (x + 0.044715 x^3): f' = s + x s (1 - s) z'(x).  At the real GELU the
                        slope is Phi(x) + x phi(x) with maximum Phi(sqrt 2) + sqrt 2 phi(sqrt 2) = 0.92135 + 0.20755 = 1.1289 at
                        x = sqrt 2; the tanh form's maximum is 1.1290 at x = 1.412 (test_gemm_refs_cpu.py evaluates both slopes on
                        a grid of 2^-10)  ->  L = 1.13.
* `vt32_layout(y, kv_len)`: the [N, kv_pad] image gf_linear_vt32 writes of y [kv_len, N], from the header's words: inside every group
  of 32 keys, key 4 g + i (i < 4) sits at position 8 g + i and key 16 + 4 g + i at 8 g + 4 + i; zeros from kv_len to kv_pad.
* `gemm_f32(...)`: the same chain with the sum in fp32 in a stated order — K tiles of `ktile` elements (64; fp8: 128), two half-tile
  sub-steps each, column tile j (128 columns) optionally started at tile (stagger j) mod nk — and the epilogue in fp32 torch: what a
  right kernel computes up to the order inside a sub-step (fp8 operands with `mfma=`: on the accumulator of `mfma_fp8`, the restatement
  of what the fp8 MFMA instruction adds).  `fault=` injects one of FAULTS; tests/test_gemm_refs_cpu.py shows that the
  restatement passes the bars below on every random input of the GPU test, in both K orders, and that each fault does not.

The two bars (`judge` / `assert_pinned`), both against the chain, no element left out:
  (a) differing bits.  The share of elements whose bf16 BITS differ from the chain is at most 2^-10 over the whole output (where
      2^-10 numel < 1 the bits must be equal), and in every row and every column the COUNT of differing elements is at most cap(n),
      the smallest c with P[Binomial(n, 2^-10) > c] < 1e-9 (n the row's / column's length).  Derivation: a right kernel differs from
      the chain only where an fp32 pre-rounding value lies within its own evaluation error of a bf16 rounding boundary.  The fp32
      sum of K exact products is off by at most K 2^-23 S (below), typically ~sqrt(K) 2^-24 |acc|; half a bf16 spacing is 2^-9 ..
      2^-8 of the value, so a stage flips with probability ~sqrt(K) 2^-24 / 2^-9 = sqrt(K) 2^-15 (2^-12 at K = 64, 2^-10.5 at
      K = 1024 — the longest K a random case uses is 1024 for that reason), and a flipped first stage mostly survives the later
      ones.  2^-10 is at least 4 x that; the caps are the same rate asked of every row and column with a one-in-10^9 tail, which
      is what catches ONE wrong row among thousands (the whole-tensor share moves by 1 / rows).  These are conditions, not
      measurements: the restatement's worst share over the GPU test's inputs is 1.2e-4 (worst ratio of (b): 0.97).
  (b) every element:  |got - chain| <= 2^-7 m + L (K 2^-23 S + T)        (T = 0 for bf16 operands).
      2^-7 m is one bf16 step at the largest stage value — what ONE flipped rounding can cost after the operations behind it (a
      cancelling residual add keeps the step's absolute size; a multiply by |gate| or |resid| scales the step and the stage alike).
      CORRECTED from the first derivation, which took m as the largest stage value alone: a step of y (<= 2^-7 |y|) reaches the next
      stage through its slope and is then ROUNDED AGAIN, and the two roundings of the neighbouring pre-images may fall to opposite
      sides — one more step of that stage (<= 2^-7 of its value).  So a single flip of the first rounding costs up to
      2^-7 (slope |y| + |next stage| + ...), the sums listed under m, which can reach twice the largest stage.  With the largest stage
      alone the fp32 restatement — a right computation — had 1 element in ~400 000 outside at four of the GPU test's shapes (GELU at
      513 x 776 x 128 and x 320, the gate at 768 x 264 x 128: 1.18 to 1.30 of that allowance, each two bf16 values off after a
      flipped first rounding); tests/forward_refs.py records the same effect for LayerNorm's second and third rounding.
      L K 2^-23 S: the products of two bf16 (8 x 8 significant bits) or e4m3 (4 x 4) values are exact in fp32, every partial sum is at
      most S in magnitude, and each of the K additions (the K - 1 of the sum, and the bias add; the row scale's multiply rounds a value
      <= S once more and is covered by the same count because the first "addition" to a zero accumulator is exact) rounds by at most one
      fp32 ulp of its result, 2^-23 S — to nearest or truncating, in any order, with or without intermediate fused steps.  The term is
      derived, not fitted, and holds for an accumulation order inside the MFMA that nobody has documented.  It reaches the output
      through the epilogue's slope L.  Non-finite `got` is outside.
  fp8, CORRECTED: the premise "exact products added in fp32" does not hold for v_mfma_f32_16x16x128_f8f6f4.  The instruction adds the
      products of 8 consecutive k after aligning them to the group's largest exponent and truncating 13 bits below it (`mfma_fp8`,
      which restates it bit for bit): a product 2^-14 of its neighbour vanishes, whatever fp32 could hold, and the truncation is
      biased towards zero.  On the Gaussian class that moves 4 to 6 in 1000 outputs across a bf16 rounding boundary (4.5e-3 at
      K = 128, both fp8 kernels, and the same elements under every K rotation), five times the 2^-10 of (a), through no fault of a
      kernel.  So for fp8 operands
        (b) gains the derived term T (at most one truncation unit per product but the largest of its group), against the SAME
            fp64 chain of the exact product — the contract (include/goalforce.h) is unchanged; and
        (a) compares the bits with the chain evaluated on the accumulator the instruction forms (Ref.bits): what is left between a
            right kernel and that is the fp32 noise (a) was derived for, and the cap stays 2^-10 with the same row and column
            caps.  The share against the exact chain is printed beside it.
  Neither is fitted to the code under test.
"""
import collections
import functools
import math

import torch

from forward_refs import act_ref, bf16_steps, bits, rb  # noqa: F401  (re-exported)

BF = torch.bfloat16
E4M3 = torch.float8_e4m3fn
SHARE_CAP = 2.0 ** -10
TAIL = 1e-9
SMALL = 4096                              # outputs below this are drawn clear of the rounding boundaries (gauss_inputs)
REL_M = 2.0 ** -7
ULP32 = 2.0 ** -23
L_GELU, L_SILU = 1.13, 1.1
EPI_BIAS, EPI_GELU, EPI_GATE_RESID, EPI_RESID, EPI_SILU, EPI_MUL = range(6)
EPIS = tuple(range(6))
EPI_NAMES = ("bias", "gelu", "gate_resid", "resid", "silu", "mul")
FAULTS = ("row_2pct", "bias_piece_shift", "drop_last_ktile", "no_first_rounding", "gate_after_resid", "row_scale_prev")
VT32_FAULTS = ("group_unpermuted", "pad_holds_bias")


# include/goalforce.h: the epilogues' plain fp32 formula v / (1 + exp(-z)) returns -0 where exp(-z) overflows (z < -ln FLT_MAX = -88.72:
# SiLU from v = -89 down, GELU-tanh from v = -10.0625 down, z = 1.59577 (v + 0.044715 v^3) = -88.76 there and -87.3 at -10) while
# bf16(function) is not yet zero (its last values are denormal: SiLU(-97) = -7.2e-41, GELU(-10.3125) = -9.2e-41, bf16's smallest; one
# bf16 value further both round to -0).  The header said -96 and -10.25 until the GPU test walked every value.
TAILS = {EPI_SILU: (-97.0, -88.7), EPI_GELU: (-10.3125, -10.06)}


def tail_mask(y, epi):
    lo, hi = TAILS[epi]
    return (y.double() >= lo) & (y.double() <= hi)


def vals(t):
    """The fp64 values of an operand: bf16 / fp32 as they are, uint8 as OCP e4m3 codes."""
    if t.dtype == torch.uint8:
        return t.view(E4M3).float().double()
    return t.double()


def product(a, w):
    av, wv = vals(a), vals(w)
    return av @ wv.t(), av.abs() @ wv.abs().t()


def chain(acc, bias, epi, resid, gate, row_scale=None, S=None):
    acc = acc.double()
    rs = 1.0 if row_scale is None else row_scale.double()[:, None]
    lin = acc * rs
    m = lin.abs()
    if bias is not None:
        m = torch.maximum(m, bias.double().abs().expand_as(lin))
        lin = lin + bias.double()
    y = rb(lin)
    m = torch.maximum(m, y.abs())
    L = torch.ones_like(y)
    if epi in (EPI_GELU, EPI_SILU):
        out = rb(act_ref(y, "gelu_tanh" if epi == EPI_GELU else "silu"))
        out = torch.where(tail_mask(y, epi), torch.full_like(out, -0.0), out)      # the header's documented tail: -0
        L = L * (L_GELU if epi == EPI_GELU else L_SILU)
        bud = L * y.abs()                                            # a step of y through the activation's slope
    elif epi == EPI_GATE_RESID:
        t = rb(gate.double() * y)
        m = torch.maximum(torch.maximum(m, t.abs()), resid.double().abs())
        out = rb(resid.double() + t)
        L = gate.double().abs().expand_as(y).clone()
        bud = L * y.abs() + t.abs()                                  # a step of y through the gate, and t rounded again
    elif epi == EPI_RESID:
        m = torch.maximum(m, resid.double().abs())
        out = rb(resid.double() + y)
        bud = y.abs()
    elif epi == EPI_MUL:
        m = torch.maximum(m, resid.double().abs())
        out = rb(y * resid.double())
        L = resid.double().abs().clone()
        bud = L * y.abs()
    else:
        assert epi == EPI_BIAS, epi
        out = y
        bud = torch.zeros_like(y)
    m = torch.maximum(torch.maximum(m, out.abs()), bud + out.abs())
    S = torch.zeros_like(y) if S is None else S.double() * rs
    return out, m, S, L


def vt_positions(kv_pad):
    """pos[s]: where key s sits in its row of the vt32 image."""
    s = torch.arange(kv_pad)
    r = s % 32
    g, i = (r % 16) // 4, r % 4
    return (s - r) + 8 * g + i + 4 * (r // 16)


def vt32_layout(y, kv_len, fault=None, bias=None):
    """y [kv_len, N] -> [N, kv_pad] (kv_pad = kv_len rounded up to 64)."""
    assert y.shape[0] == kv_len
    kvp = -(-kv_len // 64) * 64
    out = torch.zeros((y.shape[1], kvp), dtype=y.dtype)
    pos = vt_positions(kvp)
    if fault == "group_unpermuted":                 # the last 32-key group that holds a key keeps the keys in their own order
        g0 = (kv_len - 1) // 32 * 32
        pos[g0:g0 + 32] = torch.arange(g0, g0 + 32)
    if fault == "pad_holds_bias" and kvp > kv_len:
        out[:, pos[kv_len:]] = bias.to(y.dtype)[:, None]
    out[:, pos[:kv_len]] = y.t()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the bars
@functools.lru_cache(maxsize=None)
def cap(n, p=SHARE_CAP, tail=TAIL):
    """The smallest c with P[Binomial(n, p) > c] < tail (the upper tail summed term by term; math.comb is exact)."""
    def upper(c):
        tot = 0.0
        for i in range(c + 1, min(n, c + 400) + 1):
            t = math.exp(math.log(math.comb(n, i)) + i * math.log(p) + (n - i) * math.log1p(-p))
            tot += t
            if t < 1e-30:
                break
        return tot
    c = 0
    while upper(c) >= tail:
        c += 1
    return c


Ref = collections.namedtuple("Ref", "out m S L T bits")
Ref.__doc__ = """A reference: the chain, m, S rs, L; fp8 only (else None): T rs, the truncation bound of mfma_fp8, and `bits`, the chain on the
accumulator the fp8 MFMA forms — what bar (a) compares the bits with there."""


def ref_map(r, f):
    """f applied to every tensor of a Ref (a layout change)."""
    return Ref(*[None if t is None else f(t) for t in r])


def judge(got, r, K):
    """-> dict: differing / share of (a), the worst row and column counts with their caps, violations / worst ratio of (b)."""
    assert got.shape == r.out.shape == r.m.shape == r.S.shape == r.L.shape and got.dim() == 2, (got.shape, r.out.shape)
    diff = bits(got) != bits(r.out if r.bits is None else r.bits)
    rows, cols = got.shape
    row_n, col_n = diff.sum(1), diff.sum(0)
    allow = REL_M * r.m.double() + r.L.double() * ((K * ULP32) * r.S.double() + (0.0 if r.T is None else r.T.double()))
    err = (got.double() - r.out.double()).abs()
    bad = ~(err <= allow)                                           # NaN / inf in got -> bad
    ratio = torch.where(allow > 0, err / allow, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    n = got.numel()
    first = torch.nonzero(bad | diff)[:4].tolist()
    return dict(numel=n, differing=int(diff.sum()), share=int(diff.sum()) / max(n, 1), row_worst=int(row_n.max()) if n else 0,
                row_cap=cap(cols), col_worst=int(col_n.max()) if n else 0, col_cap=cap(rows), outside=int(bad.sum()),
                worst=float(ratio.max()) if n else 0.0, first=first,
                share_exact=float((bits(got) != bits(r.out)).double().mean()) if n else 0.0)


def passes(j):
    """(a passes, b passes) of a judge() result."""
    a = j["differing"] == 0 if SHARE_CAP * j["numel"] < 1 else j["share"] <= SHARE_CAP
    return a and j["row_worst"] <= j["row_cap"] and j["col_worst"] <= j["col_cap"], j["outside"] == 0


def describe(j):
    return (f"differing bits {j['differing']}/{j['numel']} = {j['share']:.2e} (cap 2^-10), worst row {j['row_worst']} (cap {j['row_cap']}), "
            f"worst column {j['col_worst']} (cap {j['col_cap']}); {j['outside']} outside 2^-7 m + L (K 2^-23 S + T), worst {j['worst']:.3g} of it"
            + (f"; share against the exact chain {j['share_exact']:.2e}" if j["share_exact"] != j["share"] else ""))


def assert_pinned(got, r, K, what):
    j = judge(got, r, K)
    print(f"PIN {what}: {describe(j)}")
    a, b = passes(j)
    assert a, f"{what}: (a) {describe(j)}; first (row, column): {j['first']}"
    assert b, f"{what}: (b) {describe(j)}; first (row, column): {j['first']}"
    return j


def old_bars(got, ref):
    """The whole-tensor bars of test_kernels_gpu.py::test_gemm_epilogues: (rel-L2 < 2e-3 and share beyond 2 bf16 steps < 5e-3, figures)."""
    g, r = got.double(), ref.double()
    e = float((g - r).norm() / r.norm().clamp_min(1e-30))
    d = (bits(got).int() - bits(ref).int()).abs()
    frac = float((d > 2).double().mean())
    return e < 2e-3 and frac < 5e-3, e, frac


# ---------------------------------------------------------------------------------------------------------------------
# the three data classes.  Each returns dict(a, w, bias, resid, gate, rs): bf16 tensors (fp8: a, w uint8 e4m3 codes, rs fp32 [M]).
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _codes(t):
    return t.to(E4M3).view(torch.uint8)


def gauss_inputs(M, N, K, seed=0, fp8=False):
    """a ~ N(0, 1), w ~ N(0, 1) / sqrt(K), bias 0.1 N(0, 1), resid and gate N(0, 1).  fp8 (the CPU stand-in for the device's
    quantisers, which the GPU test uses instead): the fp8_linear contract with one row forced to scale > 1.
    Outputs below 4096 elements — where ONE differing element is a quarter of the 2^-10 share, and below 1024 elements already outside
    bar (a), which asks for equal bits there: a right kernel still differs where a pre-rounding value lies within a few fp32 ulps of a
    rounding boundary (about one element in 10^4), so the data are drawn again until none does — until the
    restatement gives the chain's bits for all six epilogues in every summation order it can state (K tiles of 32, 64 and 128, started
    at tile 0 or rotated by 1, 2, 3 per column tile).  The selection looks at the chain and the restatement alone."""
    for attempt in range(256):
        d = _gauss_draw(M, N, K, seed + 101 * attempt, fp8)
        if M * N >= SMALL or _order_proof(d):
            return d
    raise RuntimeError(f"gauss_inputs({M}, {N}, {K}): no draw is clear of the rounding boundaries")


def _order_proof(d, epis=EPIS):
    fp8 = d["a"].dtype == torch.uint8
    for epi in epis:
        r = reference(d, epi)
        want = bits(r.out if r.bits is None else r.bits)
        for ktile in ((128,) if fp8 else (32, 64, 128)):                 # fp8: the MFMA's accumulator is stated exactly; the epilogue in fp32
            for order in ((0,) if fp8 else (0, 1, 2, 3)):
                if d["a"].shape[1] % ktile == 0 and not torch.equal(bits(gemm_f32(d["a"], d["w"], d["bias"], epi, d["resid"], d["gate"],
                                                                                     d["rs"], ktile, order, mfma=mfma_of(d)[0] if fp8 else False)), want):
                    return False
    return True


def _gauss_draw(M, N, K, seed, fp8):
    g = _gen(1000003 * seed + 7919 * M + 31 * N + K)
    a = torch.randn((M, K), generator=g).to(BF)
    w = (torch.randn((N, K), generator=g) / math.sqrt(K)).to(BF)
    d = dict(bias=(0.1 * torch.randn(N, generator=g)).to(BF), resid=torch.randn((M, N), generator=g).to(BF),
             gate=torch.randn(N, generator=g).to(BF), rs=None)
    if fp8:
        a[M // 2] = (a[M // 2].float() * 1000).to(BF)
        scale = (a.abs().amax(-1) / 448.0).clamp_min(1.0).float()     # the row maximum and its quotient are bf16 operations there
        d["rs"] = scale
        d["x"] = a                                                    # what the device's quantiser is given
        d["w_bf16"] = w
        a, w = _codes(a.float() / (scale[:, None] + 1e-8)), _codes(w)
    d.update(a=a, w=w)
    return d


def integer_inputs(M, N, K, seed=0, fp8=False):
    """Small integers, asymmetric in both operands; integer bias and resid, gate +-1; fp8: e4m3-exact integers and power-of-two row
    scales.  Every accumulator and every stage of every epilogue is exactly representable (asserted), so the summation order cannot
    matter and the chain holds the only right answer."""
    g = _gen(2000003 * seed + 7919 * M + 31 * N + K + 1)
    amax = 1 if (fp8 or K > 320) else 2
    a = torch.randint(-amax, amax + 1, (M, K), generator=g).float()
    w = torch.randint(-1, 2, (N, K), generator=g).float()
    w[:, 0] += torch.arange(N) % 3
    a[:, K - 1] += (torch.arange(M) % 2).float()
    bias = torch.randint(-4, 5, (N,), generator=g).float()
    resid = torch.randint(-2, 3, (M, N), generator=g).float()
    gate = (torch.randint(0, 2, (N,), generator=g) * 2 - 1).float()
    rs = None
    if fp8:
        rs = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (M,), generator=g)]
    d = dict(a=_codes(a) if fp8 else a.to(BF), w=_codes(w) if fp8 else w.to(BF), bias=bias.to(BF), resid=resid.to(BF), gate=gate.to(BF), rs=rs)
    acc, _ = product(d["a"], d["w"])
    assert torch.equal(vals(d["a"]), a.double()) and torch.equal(vals(d["w"]), w.double())
    lin = acc * (1.0 if rs is None else rs.double()[:, None]) + bias.double()
    assert float(lin.abs().max()) <= 250 and torch.equal(rb(lin), lin), "integer class: a stage is not exactly representable"
    assert torch.equal(rb(resid.double() + gate.double() * lin), resid.double() + gate.double() * lin)
    assert torch.equal(rb(resid.double() * lin), resid.double() * lin)
    return d


BAND = (-3, 1)        # exponents of the selector class's bf16 patterns: 2^-3 <= |v| < 2^2 (|w + bias| < 8: clear of the activations' tails)


def _band_bf16(shape, g):
    """Random bf16 bit patterns: random sign, exponent in BAND, all 7 mantissa bits random."""
    e = torch.randint(127 + BAND[0], 127 + BAND[1] + 1, shape, generator=g)
    pat = (torch.randint(0, 2, shape, generator=g) << 15) | (e << 7) | torch.randint(0, 128, shape, generator=g)
    return pat.to(torch.int32).to(torch.int16).view(BF)


def selector_k(M, K):
    """k(m): with M >= K every position of every K tile is taken; below that the rows spread over all tiles with an odd step."""
    step = max(1, K // max(M, 1)) | 1 if M < K else 1
    return (torch.arange(M) * step + (K - 1 if M == 1 else 0)) % K


def selector_inputs(M, N, K, seed=0, fp8=False):
    """Row m of A is one-hot (1.0) at column k(m): the accumulator is the single value w[n, k(m)].  W, bias, gate and resid are random
    bit patterns with exponents in BAND (fp8: random e4m3 codes of the same band, power-of-two row scales): normal numbers, no
    overflow, and every fp32 operation of the epilogue is exact before its rounding — w + bias is a multiple of 2^-10 below 2^3 (13
    bits), gate * y a product of two 8-bit significands, resid + t spans at most 2^5 .. 2^-10 or 2^2 .. 2^-20 (23 bits) — so fp64, fp32 and torch's own
    bf16 arithmetic round the same values and agree bit for bit."""
    g = _gen(3000003 * seed + 7919 * M + 31 * N + K + 2)
    km = selector_k(M, K)
    a = torch.zeros((M, K))
    a[torch.arange(M), km] = 1.0
    if fp8:
        e = torch.randint(7 + BAND[0], 7 + BAND[1] + 1, (N, K), generator=g)
        w = ((torch.randint(0, 2, (N, K), generator=g) << 7) | (e << 3) | torch.randint(0, 8, (N, K), generator=g)).to(torch.uint8)
        rs = torch.tensor([0.25, 0.5, 1.0])[torch.randint(0, 3, (M,), generator=g)]          # |w rs| < 4 as for bf16
    else:
        w, rs = _band_bf16((N, K), g), None
    return dict(a=_codes(a) if fp8 else a.to(BF), w=w, bias=_band_bf16((N,), g), resid=_band_bf16((M, N), g), gate=_band_bf16((N,), g),
                rs=rs, k=km)


def selector_acc(d):
    """The exact accumulator of the selector class without a product: w[n, k(m)]."""
    return vals(d["w"])[:, d["k"]].t().contiguous()


def batched_inputs(cls, B, M, N, K):
    """(a [B, M, K], w [B, N, K]) bf16 of the three classes for gf_gemm_bf16_batched (no bias, no epilogue operands).  The gauss class
    is drawn clear of the rounding boundaries below SMALL outputs, as gauss_inputs is."""
    for attempt in range(256):
        a, w = _batched_draw(cls, B, M, N, K, attempt)
        if cls != "gauss" or B * M * N >= SMALL or all(_order_proof(dict(a=a[b], w=w[b], bias=None, resid=None, gate=None, rs=None), (EPI_BIAS,))
                                                       for b in range(B)):
            return a, w
    raise RuntimeError(f"batched_inputs({B}, {M}, {N}, {K}): no draw is clear of the rounding boundaries")


def _batched_draw(cls, B, M, N, K, attempt):
    g = _gen(4000003 * B + 7919 * M + 31 * N + K + 1009 * attempt)
    if cls == "integers":
        a = torch.randint(-2, 3, (B * M, K), generator=g).float()
        w = torch.randint(-1, 2, (B * N, K), generator=g).float()
        w[:, 0] += torch.arange(B * N) % 3
        a[:, K - 1] += (torch.arange(B * M) % 2).float()
    elif cls == "selector":
        a = torch.zeros((B * M, K))
        a[torch.arange(B * M), selector_k(B * M, K)] = 1.0
        w = _band_bf16((B * N, K), g)
    else:
        a, w = torch.randn((B * M, K), generator=g), torch.randn((B * N, K), generator=g) / math.sqrt(K)
    return a.to(BF).view(B, M, K), w.to(BF).view(B, N, K)


def batched_reference(a, w):
    """The Ref of a batched product, the batches' rows one after the other: [B M, N]."""
    a3, w3 = a.double(), w.double()
    B, M, _ = a3.shape
    acc = torch.einsum("bmk,bnk->bmn", a3, w3).reshape(B * M, -1)
    S = torch.einsum("bmk,bnk->bmn", a3.abs(), w3.abs()).reshape(B * M, -1)
    return Ref(*chain(acc, None, EPI_BIAS, None, None, None, S), None, None)


INPUTS = dict(gauss=gauss_inputs, integers=integer_inputs, selector=selector_inputs)


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 restatement, with the faults
def _act_f32(y, epi):
    if epi == EPI_SILU:
        return y / (1.0 + torch.exp(-y))
    z = 2.0 * torch.tensor(0.7978845608028654, dtype=torch.float32) * (y + torch.tensor(0.044715, dtype=torch.float32) * y * y * y)
    return y / (1.0 + torch.exp(-z))


def _decode_e4m3(c):
    """codes -> (signed integer significand, exponent): value = significand * 2^(exponent - 3); denormals have exponent -6."""
    c = c.to(torch.int32)
    ef, mf = (c >> 3) & 0xF, c & 7
    return torch.where((c >> 7) > 0, -1, 1) * torch.where(ef > 0, mf + 8, mf), torch.clamp(ef, min=1) - 7


def mfma_fp8(a8, w8):
    """(acc, T): what v_mfma_f32_16x16x128_f8f6f4 accumulates of e4m3 codes, and a bound of its distance from the exact product.
    The instruction does NOT add exact products in fp32.  This is a model MEASURED on the MI355X through the two fp8 kernels (no vendor
    document states it): probes with one large product beside small ones gave the group size, the reference exponent and the width,
    and the model then reproduces the kernels' outputs — the 8-wave kernel bit for bit, the 4-wave kernel to within one element in
    32 768 on random codes over the whole e4m3 range (the model adds the group sums exactly, the kernel in fp32 in its own order),
    and every one of the 284 Gaussian comparisons of the GPU test with no differing element.
    tests/test_gemm_pinned_gpu.py::test_fp8_mfma_model holds it:
    the K index is cut into groups of 8 consecutive k; inside a group every product (an 8-bit integer significand times
    2^(ea + ew - 6)) is aligned to the group's largest exponent SUM E = max(ea + ew) over its non-zero products and TRUNCATED towards
    zero to a multiple of 2^(E - 13); the truncated products are added exactly and the group sums are accumulated (to fp32
    precision).  A product 2^-14 of its group's largest is dropped whole.
    T = sum over the groups that hold a non-zero product of 7 x 2^(E - 13): every product but one of the largest exponent sum loses
    less than 2^(E - 13)."""
    ma, ea = _decode_e4m3(a8)
    mw, ew = _decode_e4m3(w8)
    (M, K), N = a8.shape, w8.shape[0]
    # significand * 2^exponent per operand (exact in fp32, and so is the product of two: 8 significant bits); a zero operand takes
    # no part in the group's largest exponent sum
    A, W = ma.float() * torch.exp2(ea.float()), mw.float() * torch.exp2(ew.float())
    EA, EW = torch.where(ma != 0, ea, -64).float(), torch.where(mw != 0, ew, -64).float()
    acc, T = torch.zeros((M, N), dtype=torch.float64), torch.zeros((M, N), dtype=torch.float64)
    for g in range(0, K, 8):
        emax = (EA[:, None, g:g + 8] + EW[None, :, g:g + 8]).amax(-1)                      # [M, N]; below -60: the group is all zero
        live = emax > -60
        emax = torch.where(live, emax, torch.zeros_like(emax))
        kept = torch.trunc(A[:, None, g:g + 8] * W[None, :, g:g + 8] * torch.exp2(7 - emax)[..., None])   # = pm 2^(es - E + 7): units of 2^(E - 13)
        unit = torch.exp2(emax.double() - 13)
        acc += kept.sum(-1).double() * unit
        T += 7.0 * unit * live
    return acc, T


def mfma_of(d):
    """mfma_fp8 of an input dict's operands, computed once."""
    if "_mfma" not in d:
        d["_mfma"] = mfma_fp8(d["a"], d["w"])
    return d["_mfma"]


def sum_f32(a, w, ktile=64, stagger=0, fault=None):
    """A W^T in fp32: per column tile of 128, the K tiles in order from tile (stagger j) mod nk, two half-tile sub-steps each."""
    av, wv = vals(a).float(), vals(w).float()
    M, K = av.shape
    N = wv.shape[0]
    nk, half = K // ktile, ktile // 2
    acc = torch.zeros((M, N), dtype=torch.float32)
    for j in range(-(-N // 128)):
        c = slice(128 * j, min(N, 128 * j + 128))
        k0 = (stagger * j) % nk
        tiles = [(k0 + t) % nk for t in range(nk)]
        if fault == "drop_last_ktile" and j == min(1, -(-N // 128) - 1):
            tiles = tiles[:-1]
        part = torch.zeros((M, c.stop - c.start), dtype=torch.float32)
        for t in tiles:
            for h in range(2):
                ks = slice(t * ktile + h * half, t * ktile + (h + 1) * half)
                part = part + av[:, ks] @ wv[c, ks].t()
        acc[:, c] = part
    return acc


def gemm_f32(a, w, bias, epi, resid, gate, row_scale=None, ktile=64, order=0, fault=None, mfma=False):
    """-> bf16 [M, N].  `order`: the stagger of the K-loop rotation (0: every column tile starts at K tile 0)."""
    f = lambda t: t.float()          # noqa: E731
    acc = sum_f32(a, w, ktile, order, fault)
    if mfma is not False and a.dtype == torch.uint8 and fault != "drop_last_ktile":     # the fp8 MFMA's own accumulator (True, or given)
        acc = (mfma_fp8(a, w)[0] if mfma is True else mfma).float()
    M, N = acc.shape
    if fault == "row_2pct":
        acc[M // 2] = acc[M // 2] * 1.02
    if row_scale is not None:
        rs = f(row_scale)
        if fault == "row_scale_prev":
            rs = torch.cat([rs[:1], rs[:-1]])
        acc = acc * rs[:, None]
    b = torch.zeros(N) if bias is None else f(bias).clone()
    lin = acc + b
    if fault == "bias_piece_shift":                                  # one store piece: 8 columns of one row
        r, c = M // 3, 8 * ((N // 8) // 2 - 1) if N >= 24 else 0
        lin[r, c:c + 8] = acc[r, c:c + 8] + b[c + 8:c + 16]
    y = lin if (fault == "no_first_rounding" and epi in (EPI_GELU, EPI_SILU, EPI_GATE_RESID)) else rb(lin)
    if epi in (EPI_GELU, EPI_SILU):
        out = _act_f32(y, epi)
    elif epi == EPI_GATE_RESID:
        out = f(gate) * rb(f(resid) + y) if fault == "gate_after_resid" else f(resid) + rb(f(gate) * y)
    elif epi == EPI_RESID:
        out = f(resid) + y
    elif epi == EPI_MUL:
        out = y * f(resid)
    else:
        out = y
    return out.to(BF)


def reference(d, epi):
    """The Ref of an input dict (cached by the callers).  The selector class takes its accumulator without a product; fp8 products
    (other than the selector's single one) get the MFMA's truncation bound and the chain on the MFMA's accumulator."""
    if "k" in d:
        return Ref(*chain(selector_acc(d), d["bias"], epi, d["resid"], d["gate"], d["rs"]), None, None)
    acc, S = product(d["a"], d["w"])
    r = chain(acc, d["bias"], epi, d["resid"], d["gate"], d["rs"], S)
    if d["a"].dtype != torch.uint8:
        return Ref(*r, None, None)
    acc8, T = mfma_of(d)
    return Ref(*r, T * d["rs"].double()[:, None], chain(acc8, d["bias"], epi, d["resid"], d["gate"], d["rs"])[0])


# ---------------------------------------------------------------------------------------------------------------------
# the shapes both test files walk (M, N, K): covering sets — every value of each axis at least once, the extremes together
PH_CASES = [(1, 8, 64), (511, 520, 320), (15, 16, 128), (16, 24, 192), (17, 120, 256), (63, 128, 320), (64, 136, 64), (65, 248, 128),
            (127, 256, 192), (128, 264, 256), (129, 520, 320), (255, 8, 320), (256, 264, 128), (257, 264, 64), (257, 264, 192),
            (130, 264, 1024)]
A4_CASES = [(512, 8, 64), (769, 776, 320), (513, 136, 128), (527, 256, 192), (528, 264, 320), (529, 520, 64), (639, 776, 128),
            (640, 8, 192), (641, 136, 320), (767, 256, 64), (768, 264, 128)]
A4_BIG = (2305, 264, 64)                  # nine row tiles: a ragged last group of 8 (and of 4 with a4_group_m = 4)
STAGGER_SHAPE = (513, 776)                # four column tiles: the rotation wraps at nk = 3 and 5 and is 0 for every tile at nk = 1 and 2
STAGGERS = (0, 1, 2, 3)
BF16_K = (64, 128, 192, 320)
F8_CASES = [(1, 8, 128), (511, 520, 640), (15, 16, 256), (16, 24, 384), (17, 120, 640), (63, 128, 128), (64, 136, 256), (65, 248, 384),
            (127, 256, 640), (128, 264, 128), (129, 520, 256), (255, 8, 384), (256, 264, 640), (257, 264, 128)]
A4F8_CASES = [(512, 8, 128), (769, 776, 640), (513, 136, 256), (527, 256, 384), (528, 264, 640), (529, 520, 128), (639, 776, 256),
              (640, 8, 384), (641, 136, 640), (767, 256, 128), (768, 264, 256)]
A4F8_BIG = (2305, 264, 128)
FP8_K = (128, 256, 384, 640)
VT_KV = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 513)
VT_CASES = [(kv, (512, 640, 768)[i % 3], (64, 192, 320)[(i + i // 3) % 3]) for i, kv in enumerate(VT_KV)]          # (kv_len, N, K)
VT_CASES_FP8 = [(kv, (512, 640, 768)[i % 3], (128, 384)[(i + i // 3) % 2]) for i, kv in enumerate(VT_KV)]
BATCHED_CASES = [(1, 1, 8, 64), (3, 257, 120, 128), (40, 513, 128, 64), (3, 1, 136, 192), (40, 257, 264, 64), (1, 513, 264, 128),
                 (3, 513, 8, 64), (40, 1, 120, 128)]                                                                 # (batch, M, N, K)
