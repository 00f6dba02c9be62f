"""Exact chains, fp32 restatements and the two bars of the forward row and elementwise kernels (goal_force_amd/csrc/gf_rowops.hip,
gf_elementwise.hip).  Plain helper: CPU tensors in, CPU tensors out, no GPU and no project import.

* `*_chain`: the reference's sequence of operations with every reduction and every arithmetic step in fp64 and a rounding to bf16 at
  exactly the points where include/goalforce.h and the kernel comments say the reference rounds:
      LayerNorm   after the normalise (+ affine), after `* (1 + scale)`, after `+ shift`;
      RMSNorm     after `x * rstd`, after `* weight`, after the rotation;
      rope_apply  after the rotation;   SiLU / GELU-tanh  once, at the end.
  Each returns (chain as fp64 holding bf16 values, m), m per element: the largest magnitude among that element's stage values and
  the operands of its last addition (the bias / shift add, the two products of a rotated component).
  With `budget=True` (tools/fuzz_ops.py's large random shapes only, never the tests) m is raised to the element's ulp budget where
  that is larger: every rounding stage may land one bf16 value off (one ulp <= 2^-7 of that stage's value), and what the stages
  before it were off by reaches it through the operation in between — times |1 + scale| or |weight| through a multiply, unchanged
  through an add, times |cos| and |sin| of the two components through the rotation:
      LayerNorm  |s1|  ->  |s1| |1 + scale| + |s2|  ->  ... + |s3|;     RMSNorm  |n| |w| + |y|  ->  rotated + |out|.
  For a chain with one rounding the budget IS the stage value.
* `*_f32`: the same chain with the reductions and the arithmetic in fp32 torch — what a right kernel computes, up to the order of its
  sums.  `fault=` injects one of FAULTS; tests/test_forward_refs_cpu.py shows that the restatements pass the bars below on every input
  the GPU test uses, and that each fault does not.
* The bars (`judge` / `assert_pinned`), both against the chain, no element left out:
    (a) the share of elements whose bf16 BITS differ from the chain is at most 2^-10.  A right kernel differs only where an fp32
        pre-rounding value lies within its own evaluation error of a bf16 rounding boundary: a few fp32 ulps (<= 16 for statistics over
        <= 8192 terms) against half a bf16 spacing, 2^-8 relative: 16 * 2^-24 / 2^-8 = 2^-12 per stage, at most three stages.  Where
        2^-10 * numel < 1 the bits must be equal.
    (b) every element:  |got - chain| <= 2^-7 m + 2^-16 s,  s the rms of the chain's row.  2^-7 m is one bf16 ulp at the largest
        stage feeding the element (what ONE flipped rounding can cost after a cancelling add); 2^-16 s is ~128 fp32 epsilons of the
        row's magnitude (fp32 evaluation in another order, the term tests/backward_refs.py uses: `y w + b` may cancel BEFORE its only
        rounding).  Non-finite `got` is outside.  The fp32 restatement has no element outside on any input the GPU test uses
        (worst 0.92 of the allowance for LayerNorm, 0.37 for RMSNorm + RoPE).  At 515 x 5120 it has 1 to 3 elements outside (worst
        1.47x; 1 at 129 x 1536) for the LayerNorm operand sets with two or three roundings: a stage-1 flip of one ulp, carried through
        `* (1 + scale)` or `+ shift`, is rounded AGAIN and may come out two values off — one element in a million, which the 13-row
        cases do not meet.  The fuzzer, whose shapes are that large, therefore judges with `budget=True`.
  Neither is fitted to the code under test.
* The activations are a function of one bf16 value, so their bar is the format's: at most one bf16 step from bf16(fp64 function) on
  every finite input, differing share <= 2^-10 (`act_judge`).
"""
import math

import torch

from backward_refs import rope_table  # noqa: F401  (re-exported: the tables of both test files)

BF = torch.bfloat16
SHARE_CAP = 2.0 ** -10
REL_M = 2.0 ** -7
ABS_S = 2.0 ** -16
FAULTS = ("dropped_rounding", "scale_for_1p_scale", "rope_pair_without_mod", "mean_drops_last_8", "rope_sin_sign")
OPERANDS = ("weight", "bias", "scale1p", "shift")
SUBSETS = [tuple(n for i, n in enumerate(OPERANDS) if k >> i & 1) for k in range(16)]
DIT_SETS = [(), ("weight", "bias"), ("scale1p", "shift")]          # the three operand sets the DiT uses


def rb(t):
    """Round to bf16 (nearest even) and return in the dtype it came in."""
    return t.to(BF).to(t.dtype)


def bits(t):
    return t.to(BF).contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------------
# the bars
def judge(got, chain, m):
    """-> dict(share, differing, outside, worst, numel): the differing-bits share of (a) and the violations / worst ratio of (b)."""
    assert got.shape == chain.shape == m.shape, (got.shape, chain.shape, m.shape)
    chain, m = chain.double(), m.double()
    differing = int((bits(got) != bits(chain)).sum())
    s = chain.reshape(-1, chain.shape[-1]).pow(2).mean(-1, keepdim=True).sqrt().reshape(chain.shape[:-1] + (1,))
    allow = REL_M * m + ABS_S * s
    err = (got.double() - chain).abs()
    bad = ~(err <= allow)                                           # NaN / inf in got -> bad
    ratio = torch.where(allow > 0, err / allow, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    n = chain.numel()
    return dict(share=differing / max(n, 1), differing=differing, outside=int(bad.sum()), worst=float(ratio.max()) if n else 0.0, numel=n)


def passes(j):
    """(a passes, b passes) of a judge() result."""
    a = j["differing"] == 0 if SHARE_CAP * j["numel"] < 1 else j["share"] <= SHARE_CAP
    return a, j["outside"] == 0


def assert_pinned(got, chain, m, what):
    j = judge(got, chain, m)
    print(f"PIN {what}: differing bits {j['differing']}/{j['numel']} = {j['share']:.2e} (cap 2^-10 = {SHARE_CAP:.2e}); "
          f"{j['outside']} outside 2^-7 m + 2^-16 s, worst {j['worst']:.3f} of the allowance")
    a, b = passes(j)
    assert a, f"{what}: (a) {j['differing']} of {j['numel']} elements differ in their bf16 bits from the exact chain (cap 2^-10)"
    assert b, f"{what}: (b) {j['outside']} of {j['numel']} elements outside 2^-7 m + 2^-16 s (worst {j['worst']:.2f}x)"
    return j


def bf16_steps(a, b):
    """Distance of two bf16 tensors in representable values (+0 and -0 are the same point); non-finite anywhere -> a huge number."""
    def line(t):
        i = bits(t).to(torch.int32) & 0xFFFF
        return torch.where(i >= 0x8000, 0x8000 - i, i)             # sign-magnitude -> a monotone integer line
    d = (line(a) - line(b)).abs()
    fin = torch.isfinite(a.float()) & torch.isfinite(b.float())
    return torch.where(fin, d, torch.full_like(d, 1 << 20))


def act_judge(got, x, kind):
    """gf_act on bf16 x against bf16(fp64 function): finite inputs -> (share of differing bits, worst distance in bf16 steps)."""
    fin = torch.isfinite(x.float())
    want = rb(act_ref(x[fin], kind))
    steps = bf16_steps(got[fin], want)
    return float((steps != 0).double().mean()), int(steps.max())


def assert_act(got, x, kind, what):
    share, worst = act_judge(got, x, kind)
    print(f"PIN {what}: differing share {share:.2e} (cap 2^-10), worst {worst} bf16 step(s) (bar 1)")
    assert worst <= 1, f"{what}: {worst} bf16 steps from bf16(fp64 {kind})"
    assert share <= SHARE_CAP, f"{what}: differing share {share:.2e} > 2^-10"


def value_class(t):
    """0 finite non-zero, 1 +0, 2 -0, 3 +inf, 4 -inf, 5 NaN — what a special input must share with torch's CPU result."""
    f = t.float()
    neg = torch.signbit(f)
    c = torch.zeros(f.shape, dtype=torch.int8)
    c[(f == 0) & ~neg], c[(f == 0) & neg] = 1, 2
    c[torch.isposinf(f)], c[torch.isneginf(f)], c[torch.isnan(f)] = 3, 4, 5
    return c


# ---------------------------------------------------------------------------------------------------------------------
# inputs and the cases both test files walk
def _gen(seed):
    return torch.Generator().manual_seed(seed)


SPECIAL_ROWS = dict(constant=2, zero=5, offset=7, scaled=9)          # row numbers in a 13-row input


def offset_row(dim, generator, offset=300.0, sigma=16.0):
    """bf16(offset + sigma * noise), drawn again until no value of its plain normalisation lies close to a bf16 rounding boundary.
    Why: at offset 300 bf16 has a spacing of 2, so the row takes only ~50 distinct values and one of them is up to 5% of the row; and the
    premise of bar (a) — an evaluation error of a few fp32 ulps OF THE VALUE — does not hold for x - mean here: the mean of a right
    fp32 kernel is off by up to an fp32 ulp of 300 (3e-5, whether it divides the exact sum or multiplies it by the rounded 1 / dim),
    which x - mean keeps in full and rstd scales.  A value within that distance of a boundary may round either way in a right kernel
    and would take its whole class with it; the margin asked for is four times that."""
    for _ in range(256):
        row = (offset + sigma * torch.randn((dim,), generator=generator)).to(BF)
        xd = row.double()
        t = xd - xd.mean()
        rstd = 1.0 / math.sqrt(float(t.pow(2).mean()) + 1e-6)
        y = (t * rstd).abs()
        ulp = torch.exp2(torch.floor(torch.log2(y.clamp_min(1e-300))) - 7)      # bf16 spacing at y
        frac = y / ulp
        dist = ((frac - torch.floor(frac)) - 0.5).abs() * ulp                      # to the nearest midpoint of two bf16 values
        if float(dist.min()) >= 4 * offset * 2.0 ** -23 * rstd:
            return row
    raise RuntimeError("offset_row: no draw keeps its values clear of the rounding boundaries")


def row_x(rows, dim, generator, special="ln"):
    """bf16 x [rows, dim].  With 13 rows or more: LayerNorm inputs get a constant row (variance 0: 2.5 sums exactly), an all-zero row,
    a row of 300 + noise (cancellation in x - mean; offset_row) and a row scaled by 1e3; RMSNorm inputs ('rms') get the all-zero row
    (rstd = 1/sqrt(eps)) and the scaled one."""
    x = torch.randn((rows, dim), generator=generator) * 1.5 + 0.3
    if rows >= 13:
        x[SPECIAL_ROWS["zero"]] = 0.0
        x[SPECIAL_ROWS["scaled"]] *= 1e3
        if special == "ln":
            x[SPECIAL_ROWS["constant"]] = 2.5
            x[SPECIAL_ROWS["offset"]] = offset_row(dim, generator).float()
    return x.to(BF)


def ln_vectors(dim, generator, subset):
    """The four bf16 vectors (all drawn, so that a subset does not change the others' values); those not in `subset` are None."""
    v = dict(weight=(1 + 0.2 * torch.randn(dim, generator=generator)).to(BF), bias=(0.1 * torch.randn(dim, generator=generator)).to(BF),
             scale1p=(1 + (0.3 * torch.randn(dim, generator=generator)).to(BF).float()).to(BF),
             shift=(0.5 * torch.randn(dim, generator=generator)).to(BF))
    return {k: (t if k in subset else None) for k, t in v.items()}


LN_GENERAL = (8, 264, 2048, 8192)      # layernorm_modulate_kernel: 264 one ragged pass, 2048 two chunks per thread, 8192 the limit
LN_WAVE = (1536, 4096, 5120)           # layernorm_wave2_kernel for DIT_SETS, layernorm_modulate_wave_kernel<NCH, OUT> for every other set
ROWS = (1, 13)                         # 13: a ragged last workgroup of the wave kernels (4 rows each)


def ln_cases():
    """(rows, dim, subset): all 16 subsets at one general and one wave width, the three DiT sets at every width."""
    out = []
    for dim in LN_GENERAL + LN_WAVE:
        for sub in (SUBSETS if dim in (264, 5120) else DIT_SETS):
            out += [(rows, dim, sub) for rows in ROWS]
    return out


def ln_inputs(rows, dim, subset):
    g = _gen(7 * dim + rows)
    return row_x(rows, dim, g), ln_vectors(dim, g, subset)


# (dim, head_dim or None).  General kernel (rmsnorm_rope_kernel): 8 / 264 / 2048 / 8192.  Wave kernels: None -> ROPE = 0;
# head_dim dividing 512 -> ROPE = 1; head_dim not dividing 512 -> ROPE = 2 (the table is indexed per chunk).
RMS_SHAPES = [(8, None), (8, 8), (264, None), (264, 8), (264, 88), (2048, None), (2048, 128), (2048, 64), (8192, None), (8192, 128),
              (8192, 1024),
              (1536, None), (4096, None), (5120, None),
              (5120, 128), (5120, 64), (5120, 8), (4096, 128), (4096, 8), (1536, 128), (1536, 64),
              (1536, 96), (1536, 768), (5120, 40), (5120, 320), (5120, 1024), (5120, 5120), (4096, 1024), (4096, 4096)]
ROPE2_SHAPES = [(d, h) for d, h in RMS_SHAPES if h is not None and d in LN_WAVE and 512 % h != 0]
Q_PRESCALE_128 = 0.1275                # the q pre-scale at head_dim 128 (softmax scale * log2 e): a table that is not unit-modulus


def rms_cases():
    """(rows, dim, head_dim, table scale): one row with a unit-modulus table, 13 rows with a unit-modulus and a scaled one."""
    out = []
    for dim, hd in RMS_SHAPES:
        out += [(1, dim, hd, 1.0), (13, dim, hd, 1.0)] + ([(13, dim, hd, Q_PRESCALE_128)] if hd is not None else [])
    return out


def rms_inputs(rows, dim, hd, scale):
    g = _gen(11 * dim + rows + (hd or 0))
    x = row_x(rows, dim, g, "rms")
    w = (1 + 0.2 * torch.randn(dim, generator=g)).to(BF)
    cos, sin = (None, None) if hd is None else rope_table(rows, hd, g, scale)
    return x, w, cos, sin


BIG_ROPE = [(1100, 3840, 96), (1100, 3840, 128)]        # 528 000 chunks > 2048 blocks x 256: the grid-stride loops iterate


# ---------------------------------------------------------------------------------------------------------------------
# exact chains (fp64 arithmetic, bf16 roundings where the reference has them)
def layernorm_chain(x, weight=None, bias=None, scale1p=None, shift=None, eps=1e-6, budget=False):
    xd = x.double()
    mean = xd.mean(-1, keepdim=True)
    t = xd - mean
    y = t / torch.sqrt(t.pow(2).mean(-1, keepdim=True) + eps)
    if weight is not None:
        y = y * weight.double()
    m = torch.zeros_like(y)
    if bias is not None:
        if shift is None:                                                    # the operands of this add when it is the last one
            m = torch.maximum(y.abs(), bias.double().abs().expand_as(y))
        y = y + bias.double()
    y = rb(y)                                                                # .type_as(x)
    m = torch.maximum(m, y.abs())
    bud = m.clone()                                                          # the ulp budget, see the module docstring
    if scale1p is not None:
        y = rb(y * scale1p.double())                                         # x * (1 + scale)
        m = torch.maximum(m, y.abs())
        bud = bud * scale1p.double().abs() + y.abs()
    if shift is not None:
        m = torch.maximum(m, shift.double().abs().expand_as(y))
        y = rb(y + shift.double())                                           # + shift
        m = torch.maximum(m, y.abs())
        bud = bud + y.abs()
    return y, (torch.maximum(m, bud) if budget else m)


def _rotate(y, cos, sin, head_dim, pair_without_mod=False, flip_sin=False, budget=None):
    """(out, largest |product|[, the ulp budgets `budget` of y carried through]) of the complex rotation of adjacent pairs, in y's
    dtype; cos / sin [rows, head_dim/2]."""
    rows, dim = y.shape
    c, s = cos.to(y.dtype), sin.to(y.dtype)
    if flip_sin:
        s = -s
    if pair_without_mod:        # the pair index dim-wide instead of head-wide: reads on through the flat table, as the kernel's pointer would
        idx = (torch.arange(rows)[:, None] * (head_dim // 2) + torch.arange(dim // 2)[None, :]) % c.numel()
        c, s = c.flatten()[idx], s.flatten()[idx]
    else:
        c, s = c[:rows].repeat(1, dim // head_dim), s[:rows].repeat(1, dim // head_dim)
    a, b = y[:, 0::2], y[:, 1::2]
    ac, bs, as_, bc = a * c, b * s, a * s, b * c
    out = torch.stack([ac - bs, as_ + bc], -1).reshape(rows, dim)
    big = torch.stack([torch.maximum(ac.abs(), bs.abs()), torch.maximum(as_.abs(), bc.abs())], -1).reshape(rows, dim)
    if budget is None:
        return out, big
    ba, bb = budget[:, 0::2], budget[:, 1::2]                       # the incoming budgets, through |c| and |s| as the values go
    return out, big, torch.stack([ba * c.abs() + bb * s.abs(), ba * s.abs() + bb * c.abs()], -1).reshape(rows, dim)


def rmsnorm_rope_chain(x, weight, cos=None, sin=None, head_dim=128, eps=1e-6, budget=False):
    xd = x.double()
    n = rb(xd / torch.sqrt(xd.pow(2).mean(-1, keepdim=True) + eps))          # norm(x.float()).to(dtype)
    y = rb(n * weight.double())                                              # * weight
    m = torch.maximum(n.abs(), y.abs())
    bud = n.abs() * weight.double().abs() + y.abs()
    if cos is not None:
        y, big, bud = _rotate(y, cos, sin, head_dim, budget=bud)
        y = rb(y)
        m = torch.maximum(torch.maximum(m, big), y.abs())
        bud = bud + y.abs()
    return y, (torch.maximum(m, bud) if budget else m)


def rope_apply_chain(x, cos, sin, head_dim):
    y, big = _rotate(x.double(), cos, sin, head_dim)
    y = rb(y)
    return y, torch.maximum(big, y.abs())


_K0, _K1 = 0.7978845608028654, 0.044715


def act_ref(x, kind):
    """SiLU | GELU-tanh in fp64, unrounded.  Both are x * sigmoid(z) (z = x | 2 sqrt(2/pi) (x + 0.044715 x^3), the identity
    0.5 (1 + tanh u) = sigmoid(2u)), with the sigmoid evaluated without cancellation on either side."""
    xd = x.double()
    z = xd if kind == "silu" else 2.0 * _K0 * (xd + _K1 * xd ** 3)
    e = torch.exp(-z.abs())
    return xd * torch.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


# ---------------------------------------------------------------------------------------------------------------------
# fp32 restatements, with the faults
def _f(t):
    return t.float()


def layernorm_f32(x, weight=None, bias=None, scale1p=None, shift=None, eps=1e-6, fault=None):
    xf = _f(x)
    dim = x.shape[-1]
    n = dim - 8 if fault == "mean_drops_last_8" else dim
    mean = xf[:, :n].sum(-1, keepdim=True) / n
    t = xf - mean
    y = t * (1.0 / torch.sqrt((t * t).sum(-1, keepdim=True) / dim + torch.tensor(eps, dtype=torch.float32)))
    if weight is not None:
        y = y * _f(weight)
    if bias is not None:
        y = y + _f(bias)
    drop = fault == "dropped_rounding"
    if not (drop and (scale1p is not None or shift is not None)):
        y = rb(y)
    if scale1p is not None:
        y = y * (_f(scale1p) - 1.0 if fault == "scale_for_1p_scale" else _f(scale1p))
        if not (drop and shift is not None):
            y = rb(y)
    if shift is not None:
        y = rb(y + _f(shift))
    return y.to(BF)


def rmsnorm_rope_f32(x, weight, cos=None, sin=None, head_dim=128, eps=1e-6, fault=None):
    xf = _f(x)
    dim = x.shape[-1]
    n = dim - 8 if fault == "mean_drops_last_8" else dim
    rstd = 1.0 / torch.sqrt((xf * xf)[:, :n].sum(-1, keepdim=True) / n + torch.tensor(eps, dtype=torch.float32))
    y = xf * rstd
    if fault != "dropped_rounding":
        y = rb(y)
    y = rb(y * _f(weight))
    if cos is not None:
        y = rb(_rotate(y, cos, sin, head_dim, fault == "rope_pair_without_mod", fault == "rope_sin_sign")[0])
    return y.to(BF)


def rope_apply_f32(x, cos, sin, head_dim, fault=None):
    return _rotate(_f(x), cos, sin, head_dim, fault == "rope_pair_without_mod", fault == "rope_sin_sign")[0].to(BF)


def act_naive_f32(x, kind):
    """x / (1 + exp(-z)) in fp32 and nothing else: 1 + exp(-z) overflows for z < -88.7 and the result is -0, while the function is
    still a normal bf16 number (SiLU down to x = -96, GELU-tanh for -10.25 <= x <= -10.06)."""
    xf = _f(x)
    z = xf if kind == "silu" else 2.0 * torch.tensor(_K0, dtype=torch.float32) * (xf + torch.tensor(_K1, dtype=torch.float32) * xf * xf * xf)
    return (xf / (1.0 + torch.exp(-z))).to(BF)


def act_f32(x, kind):
    """act_kernel's formulas in fp32 torch: the naive one, and in the far negative tail (where 1 + exp(-z) = exp(-z) in fp32)
    x * exp(z) with the exponent shifted so that no intermediate leaves the normal range."""
    xf = _f(x)
    z = xf if kind == "silu" else 2.0 * torch.tensor(_K0, dtype=torch.float32) * (xf + torch.tensor(_K1, dtype=torch.float32) * xf * xf * xf)
    cut, shift = (-87.0, 32.0) if kind == "silu" else (-100.0 * math.log(2.0), 100.0 * math.log(2.0))
    tail = (xf * torch.exp(z + shift)) * torch.tensor(math.exp(-shift), dtype=torch.float32)
    return torch.where(z < cut, tail, xf / (1.0 + torch.exp(-z))).to(BF)


def all_bf16():
    """Every one of the 65 536 bf16 bit patterns, in pattern order."""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)


# ---------------------------------------------------------------------------------------------------------------------
# the operations that are plain bf16 eager arithmetic: torch's own CPU result is the reference, bit for bit
def cfg_euler_ref(lat, posi, nega, cfg, dsigma):
    """latents + (nega + cfg (posi - nega)) * dsigma, every op an fp32 operation on bf16 operands rounded to bf16 — what torch's eager
    bf16 arithmetic does with fp32 scalars (tests/test_forward_refs_cpu.py holds this against the eager expression)."""
    f = lambda s: torch.tensor(s, dtype=torch.float32)            # noqa: E731
    pred = posi.float()
    if nega is not None:
        pred = rb(nega.float() + rb(f(cfg) * rb(pred - nega.float())))
    return (lat.float() + rb(pred * f(dsigma))).to(BF)


def modulation_ref(param, t, onep_mask):
    """out[i] = param[i] + t[i % t_rows] in bf16; rows whose bit is set in onep_mask become 1 + out[i], rounded again."""
    k = param.shape[0]
    out = param + t[torch.arange(k) % t.shape[0]]
    rows = [i for i in range(k) if onep_mask >> i & 1]
    if rows:
        out[rows] = 1 + out[rows]
    return out


QUANT_MAXIMA = (0.0, 448.0, 450.0, 452.0, 466.0, 1500.0, 3e4)   # row maxima: scale_a = 1 up to 448, bf16(max / 448) above


def quant_inputs(rows, dim, seed):
    """bf16 x [rows, dim] whose first rows have the maxima QUANT_MAXIMA (one element set to +-max, the others strictly below it); with
    one row: the maximum 452."""
    g = _gen(seed)
    x = torch.randn((rows, dim), generator=g)
    for r, mx in enumerate(QUANT_MAXIMA if rows > 1 else (452.0,)):
        if r >= rows:
            break
        x[r] = x[r] / x[r].abs().max() * 0.98 * mx
        x[r, (5 * r + 3) % dim] = mx if r % 2 else -mx
    return x.to(BF)
