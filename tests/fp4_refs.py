"""MXFP4 (include/goalforce.h, "MXFP4 Linear") restated in torch: the quantiser, the decoder, the exact chain of gf_gemm_mxfp4 on the
dequantised operands (gemm_refs.chain / judge / assert_pinned), the data classes of the GPU test and `mfma_mxfp4`, a model of what
v_mfma_scale_f32_16x16x128_f8f6f4 accumulates of e2m1 operands.  Plain helper: CPU tensors in, CPU tensors out, no project import.

The quantiser is integer work on the bf16 bit patterns and exact power-of-two scalings in fp64, so it can be (and is, on the GPU test's
inputs) bit-identical to the kernel.  Operands travel as (packed uint8 [rows, K/2], E8M0 uint8 [rows, K/32]).
"""
import math

import torch

import gemm_refs as R
from gemm_refs import BF, EPIS, Ref, bits, rb  # noqa: F401  (re-exported)

E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)
BLOCK = 32
KTILE = 256                 # one 128-byte LDS row of gf_gemm_mxfp4 = two MFMA k-steps of 128
NAN_SCALE = 255


# ---------------------------------------------------------------------------------------------------------------------
# the format
def unpack(x4):
    """packed [rows, K/2] uint8 -> codes [rows, K] uint8 (0 .. 15): element 2i in bits 3:0 of byte i, 2i + 1 in bits 7:4."""
    return torch.stack([x4 & 0xF, x4 >> 4], -1).reshape(x4.shape[0], -1)


def pack(codes):
    c = codes.to(torch.uint8).reshape(codes.shape[0], -1, 2)
    return c[..., 0] | (c[..., 1] << 4)


def code_values(codes):
    v = E2M1[(codes & 7).long()]
    return torch.where((codes & 8) > 0, -v, v)


def scale_values(scale):
    """E8M0 -> fp64: 2^(code - 127); code 255 = NaN."""
    s = torch.exp2(scale.double() - 127.0)
    return torch.where(scale == NAN_SCALE, torch.full_like(s, math.nan), s)


def decode(x4, scale):
    """-> the fp64 values [rows, K] (NaN over a block whose scale is 255)."""
    return code_values(unpack(x4)) * scale_values(scale).repeat_interleave(BLOCK, dim=1)


def quantize(x):
    """The recipe of include/goalforce.h on a bf16 [rows, dim] tensor (dim % 32 == 0) -> (packed, scale)."""
    assert x.dtype == BF and x.dim() == 2 and x.shape[1] % BLOCK == 0, (x.dtype, x.shape)
    rows, dim = x.shape
    pat = x.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    mag = (pat & 0x7FFF).view(rows, dim // BLOCK, BLOCK)
    amax = mag.amax(-1)                                         # |x| orders like its bit pattern; NaN / inf are >= 0x7F80
    ef, mant = amax >> 7, amax & 127
    lead = torch.zeros_like(mant)                               # floor(log2 mantissa) of a subnormal maximum
    for b in range(1, 7):
        lead = torch.where(mant >= (1 << b), torch.full_like(lead, b), lead)
    fl = torch.where(ef > 0, ef - 127, lead - 133)              # floor(log2 amax)
    code = torch.clamp(fl - 2 + 127, 0, 254)
    zero, bad = amax == 0, amax >= 0x7F80
    code = torch.where(zero, torch.full_like(code, 127), code)
    v = x.double().abs().view(rows, dim // BLOCK, BLOCK) * torch.exp2((127 - code).double())[..., None]       # exact; < 8
    v = torch.where((zero | bad)[..., None], torch.zeros_like(v), v)
    c = torch.where(v < 2, torch.round(v * 2), torch.where(v < 4, 2 + torch.round(v), torch.clamp(4 + torch.round(v / 2), max=7)))
    c = c.to(torch.int32) | ((pat.view(rows, dim // BLOCK, BLOCK) >> 12) & 8)
    c = torch.where((zero | bad)[..., None], torch.zeros_like(c), c)
    code = torch.where(bad, torch.full_like(code, NAN_SCALE), code)
    return pack(c.view(rows, dim)), code.to(torch.uint8)


def fake_quant(x):
    """bf16 [rows, dim] -> the fp64 values its MXFP4 image stands for."""
    return decode(*quantize(x))


# ---------------------------------------------------------------------------------------------------------------------
# what the instruction accumulates
def _block_sums(a4, sa, w4, sw):
    """Per MX block, WITHOUT the scales: the exact sum of the products and of their magnitudes, [M, N, K/32] (multiples of 1/4 below 2^11:
    exact), and the blocks' exponents sa + sw - 254 as [M, N, K/32] fp64."""
    av, wv = code_values(unpack(a4)), code_values(unpack(w4))
    M, K = av.shape
    N = wv.shape[0]
    nb = K // BLOCK
    sums = torch.einsum("mbk,nbk->mnb", av.view(M, nb, BLOCK), wv.view(N, nb, BLOCK))
    mags = torch.einsum("mbk,nbk->mnb", av.abs().view(M, nb, BLOCK), wv.abs().view(N, nb, BLOCK))
    e = sa.double()[:, None, :] + sw.double()[None, :, :] - 254.0
    return sums, mags, e


def kloop_blocks(K):
    """The order in which gf_gemm_mxfp4 feeds the MX blocks of a row to the instruction: per K tile of 8 blocks, sub-step s takes blocks
    s, 2 + s, 4 + s, 6 + s (lane group kb holds block 2 kb + s).  Four consecutive entries = one instruction."""
    return [8 * t + 2 * kb + s for t in range(K // KTILE) for s in (0, 1) for kb in range(4)]


DROP_BELOW = 22             # a block whose scale sum lies this many binades or more below the instruction's largest may vanish whole
KEEP_BITS = 23              # the retained products are cut below 2^(largest scale sum - 23)
MODEL_NOTE = """What v_mfma_scale_f32_16x16x128_f8f6f4 does with e2m1 operands, as MEASURED on an MI355X (one instruction per wave on
lane-level data, 1 904 trials, and through gf_gemm_mxfp4); no vendor statement is relied on:
  * layout: lane l supplies row l & 15, MX block l >> 4 (32 k in its low four dwords, element e in nibble e, low nibble first) and that
    block's scale in byte `opsel` of its scale operand — exact on 64 one-hot trials with distinct scales, all four opsel values;
  * a scale code 255 makes the whole row (column) of that lane NaN, also over a block of zeros and whatever the other operand holds;
  * with the blocks' scale sums within 2^+-4 of each other and a zero accumulator the result is the exact sum rounded to fp32, to nearest
    even: 0 of 68 608 elements differ.  `mfma_mxfp4` states this — the CLOSEST model, not a reproduction:
  * with a non-zero accumulator 15 % of the fp32 results differ from that, also on narrow scales: the sum is cut at a fixed position
    near 2^(largest scale sum - 17 .. - 23) whatever the accumulator's own exponent (fixed-point alignment); after the bf16 rounding it
    shows on none of 1.6 M Gaussian outputs;
  * with scale sums spread wider, a block 22 or 23 binades below the largest scale sum of the instruction is dropped whole (23: always in
    the probes; 22: seen) and the other products lose bits below about 2^(largest scale sum - 23).  No rule tried reproduces the bits
    (per-product and per-block truncation at 22 .. 24 bits, towards zero, with and without a drop rule: 4 to 13 % of the elements of
    the wide-scale probes stay off).
  The bound T: every block that far down counted as lost, and per instruction two units of 2^(largest scale sum - 23) per product — one
  for the products, one for the accumulator cut at the same position.  Measured against it: worst 0.39 of T + half an ulp on the
  184 000 probe elements with a zero accumulator; with a random accumulator worst 1.0 of T + one ulp (of the larger of accumulator and
  result) on scale sums within 2^+-4 and 1.62 on wider ones — bar (b)'s own K 2^-23 S term allows 128 such ulps per instruction.
So bar (a) compares bits with the chain on this model's accumulator and bar (b) stays on the exact chain with T added
(gemm_refs.judge).  On operands from the quantiser (block scales of a row within a few binades) T is about one fp32 ulp of S."""


def mfma_mxfp4(a4, sa, w4, sw, blocks=None):
    """(acc, T): the closest model of what the K loop of gf_gemm_mxfp4 accumulates (MODEL_NOTE) and the derived bound of the
    instruction's distance from exact sums.  `blocks`: the MX blocks in feeding order, four per instruction (default: kloop_blocks)."""
    sums, mags, e = _block_sums(a4, sa, w4, sw)
    M, N, nb = sums.shape
    blocks = kloop_blocks(nb * BLOCK) if blocks is None else list(blocks)
    acc = torch.zeros((M, N), dtype=torch.float64)
    T = torch.zeros((M, N), dtype=torch.float64)
    for i in range(0, len(blocks), 4):
        b = blocks[i:i + 4]
        eb = e[..., b]
        emax = eb.amax(-1)
        acc = (acc + (sums[..., b] * torch.exp2(eb)).sum(-1)).float().double()          # one rounding to fp32 per instruction
        far = eb <= (emax[..., None] - DROP_BELOW)
        T += (mags[..., b] * torch.exp2(eb) * far).sum(-1) + 2 * 4 * BLOCK * torch.exp2(emax - KEEP_BITS)
    return acc, T


def product(a4, sa, w4, sw):
    """(acc, S) in fp64 of the dequantised operands: acc = A^ W^^T, S = |A^| |W^|^T."""
    av, wv = decode(a4, sa), decode(w4, sw)
    return av @ wv.t(), av.abs() @ wv.abs().t()


# ---------------------------------------------------------------------------------------------------------------------
# the data classes of tests/test_fp4_gpu.py.  Each returns dict(a4, sa, w4, sw, bias, resid, gate [, x, w_bf16, k]).
M_AXIS = (1, 15, 16, 17, 127, 129, 255, 256, 257, 513)
N_AXIS = (8, 56, 64, 248, 256, 264, 520)
K_AXIS = (256, 512, 768, 1280)
# a covering set: every value of each axis at least once, the extremes together
SHAPES = [(1, 8, 256), (513, 520, 1280), (15, 56, 512), (16, 64, 768), (17, 248, 1280), (127, 256, 256), (129, 264, 512), (255, 520, 768),
          (256, 8, 1280), (257, 56, 256), (513, 64, 512), (1, 248, 768), (257, 264, 1280)]
EXTRA_SHAPES = [(257, 264, 768), (17, 520, 256), (17, 56, 512)]       # the gauss cases of the GPU test's NaN, memory-discipline and refusal tests


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _epi_operands(M, N, g, integer=False):
    if integer:
        return dict(bias=torch.randint(-4, 5, (N,), generator=g).float().to(BF), resid=torch.randint(-2, 3, (M, N), generator=g).float().to(BF),
                    gate=(torch.randint(0, 2, (N,), generator=g) * 2 - 1).float().to(BF))
    return dict(bias=(0.1 * torch.randn(N, generator=g)).to(BF), resid=torch.randn((M, N), generator=g).to(BF), gate=torch.randn(N, generator=g).to(BF))


def _rand_codes(shape, g, nonzero=False):
    return (torch.randint(1 if nonzero else 0, 8, shape, generator=g) | (torch.randint(0, 2, shape, generator=g) << 3)).to(torch.uint8)


def selector_k(M, K):
    """f(m): with M >= 512 every one of the 256 positions of a K tile is taken in both tile parities; below that the rows spread over
    the whole K with an odd step."""
    step = max(1, K // max(M, 1)) | 1 if M < K else 1
    return (torch.arange(M) * step + (K - 1 if M == 1 else 0)) % K


def selector_inputs(M, N, K, seed=0):
    """The layout class: row m of A holds ONE nonzero element, at k = f(m); W is random nonzero codes (asymmetric), and every MX block
    of every row carries its own scale exponent, in A and in W: exactly one product per output is nonzero, so the result is exact
    whatever the accumulator does and a mis-mapped nibble, lane, block or opsel shows."""
    g = _gen(3000003 * seed + 7919 * M + 31 * N + K + 2)
    k = selector_k(M, K)
    A = torch.zeros((M, K), dtype=torch.uint8)
    A[torch.arange(M), k] = _rand_codes((M,), g, nonzero=True)
    W = _rand_codes((N, K), g, nonzero=True)
    nb = K // BLOCK
    sa = (107 + (torch.arange(M)[:, None] * 7 + torch.arange(nb)[None, :]) % 41).to(torch.uint8)      # 41 > K/32 = 40: distinct along a row
    sw = (109 + (torch.arange(N)[:, None] * 11 + 3 * torch.arange(nb)[None, :]) % 41).to(torch.uint8)  # 3 coprime to 41: distinct too
    return dict(a4=pack(A), sa=sa, w4=pack(W), sw=sw, k=k, **_epi_operands(M, N, g))


def integer_inputs(M, N, K, seed=0):
    """e2m1-grid values (A three quarters zeros) and scales 2^-3 .. 2^3 in both operands; integer bias and resid, gate +-1.  Every product
    is a multiple of 2^-8 and every partial sum stays below 2^15 (asserted on S = |A| |W|^T): 23 bits, exact in fp32 in any order, and a
    block's scale sum is at most 12 binades below its instruction's largest, far from where the instruction drops anything.  Every stage
    of every epilogue is then exact before its rounding (a bf16 value times +-1 or a small integer, or plus one), so the chain holds the
    only right answer."""
    g = _gen(2000003 * seed + 7919 * M + 31 * N + K + 1)
    A = _rand_codes((M, K), g)
    A = torch.where(torch.rand((M, K), generator=g) < 0.75, torch.zeros_like(A), A)
    A[:, K - 1] = (torch.arange(M) % 7 + 1).to(torch.uint8)            # asymmetric in both operands
    W = _rand_codes((N, K), g)
    W[:, 0] = (torch.arange(N) % 5 + 2).to(torch.uint8)
    sa = torch.randint(124, 131, (M, K // BLOCK), generator=g).to(torch.uint8)
    sw = torch.randint(124, 131, (N, K // BLOCK), generator=g).to(torch.uint8)
    d = dict(a4=pack(A), sa=sa, w4=pack(W), sw=sw, **_epi_operands(M, N, g, integer=True))
    acc, S = product(*operands(d))
    assert float(S.max()) + 4 < 2.0 ** 15, f"integer class {M} x {N} x {K}: a partial sum can reach {float(S.max()):.0f}"
    lin = acc + d["bias"].double()
    assert torch.equal(lin.float().double(), lin)
    return d


def gauss_inputs(M, N, K, seed=0):
    """a ~ N(0, 1), w ~ N(0, 1) / sqrt(K) in bf16 and their MXFP4 images by `quantize` (the GPU test takes the device quantiser's and
    asserts they are these); bias 0.1 N(0, 1), resid and gate N(0, 1).  Below gemm_refs.SMALL outputs the draw is repeated until the
    restatement gives the chain's bits for every epilogue in every order it can state (gemm_refs.gauss_inputs: bar (a) asks for equal
    bits there, and a right kernel differs where a pre-rounding value lies within a few fp32 ulps of a rounding boundary)."""
    for attempt in range(256):
        d = _gauss_draw(M, N, K, seed + 101 * attempt)
        if M * N >= R.SMALL or _order_proof(d):
            return d
    raise RuntimeError(f"gauss_inputs({M}, {N}, {K}): no draw is clear of the rounding boundaries")


def _gauss_draw(M, N, K, seed):
    g = _gen(1000003 * seed + 7919 * M + 31 * N + K)
    x = torch.randn((M, K), generator=g).to(BF)
    w = (torch.randn((N, K), generator=g) / math.sqrt(K)).to(BF)
    d = _epi_operands(M, N, g)
    (a4, sa), (w4, sw) = quantize(x), quantize(w)
    d.update(a4=a4, sa=sa, w4=w4, sw=sw, x=x, w_bf16=w)
    return d


ORDERS = ("plain", "kloop")


def _order_proof(d):
    for epi in EPIS:
        r = reference(d, epi)
        want = bits(r.out if r.bits is None else r.bits)
        for how in ORDERS + ("mfma",):
            if not torch.equal(bits(gemm_f32(d, epi, how)), want):
                return False
    return True


def operands(d):
    return d["a4"], d["sa"], d["w4"], d["sw"]


def model_of(d):
    if "_mfma" not in d:
        d["_mfma"] = mfma_mxfp4(*operands(d))
    return d["_mfma"]


def reference(d, epi):
    """The Ref (gemm_refs) of an input dict: the exact chain on the dequantised operands, the bound T of mfma_mxfp4 and the chain on the
    model's accumulator (what bar (a) compares the bits with); the layout class has one product per output and needs neither."""
    acc, S = product(*operands(d))
    r = R.chain(acc, d["bias"], epi, d["resid"], d["gate"], None, S)
    if "k" in d:
        return Ref(*r, None, None)
    acc_m, T = model_of(d)
    return Ref(*r, T, R.chain(acc_m, d["bias"], epi, d["resid"], d["gate"], None)[0])


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 restatement, with the faults
FAULTS = ("swapped_nibbles", "scales_shifted_one_block", "scale_from_next_row", "drop_last_ktile", "row_2pct", "bias_piece_shift")


def _faulty_operands(d, fault):
    a4, sa, w4, sw = operands(d)
    if fault == "swapped_nibbles":
        a4 = (a4 << 4) | (a4 >> 4)
    elif fault == "scales_shifted_one_block":
        sa = torch.roll(sa, 1, dims=1)
    elif fault == "scale_from_next_row":
        sw = torch.roll(sw, -1, dims=0)
    return a4, sa, w4, sw


def gemm_f32(d, epi, how="plain", fault=None):
    """-> bf16 [M, N]: the sum in fp32 over K tiles of 256 in two sub-steps ("plain": the blocks in their own order; "kloop": in the
    order the kernel feeds them, kloop_blocks), or the model's accumulator ("mfma"), and gemm_refs' fp32 epilogue."""
    a4, sa, w4, sw = _faulty_operands(d, fault)
    av, wv = decode(a4, sa).float(), decode(w4, sw).float()                 # exact: a 2-bit significand times a power of two
    rfault = fault if fault in R.FAULTS else None
    if how == "mfma" and rfault != "drop_last_ktile":
        return _epilogue_f32(mfma_mxfp4(a4, sa, w4, sw)[0].float(), d, epi, rfault)
    if how == "kloop":
        perm = torch.tensor([32 * b + e for b in kloop_blocks(av.shape[1]) for e in range(BLOCK)])
        av, wv = av[:, perm], wv[:, perm]
    return R.gemm_f32(av, wv, d["bias"], epi, d["resid"], d["gate"], None, KTILE, 0, rfault)


def _epilogue_f32(acc, d, epi, fault):
    """gemm_refs.gemm_f32's epilogue (and its two epilogue faults) on a given accumulator."""
    f = lambda t: t.float()          # noqa: E731
    acc = acc.clone()
    M, N = acc.shape
    if fault == "row_2pct":
        acc[M // 2] = acc[M // 2] * 1.02
    b = torch.zeros(N) if d["bias"] is None else f(d["bias"]).clone()
    lin = acc + b
    if fault == "bias_piece_shift":
        r, c = M // 3, 8 * ((N // 8) // 2 - 1) if N >= 24 else 0
        lin[r, c:c + 8] = acc[r, c:c + 8] + b[c + 8:c + 16]
    y = rb(lin)
    if epi in (R.EPI_GELU, R.EPI_SILU):
        out = R._act_f32(y, epi)
    elif epi == R.EPI_GATE_RESID:
        out = f(d["resid"]) + rb(f(d["gate"]) * y)
    elif epi == R.EPI_RESID:
        out = f(d["resid"]) + y
    elif epi == R.EPI_MUL:
        out = y * f(d["resid"])
    else:
        out = y
    return out.to(BF)
