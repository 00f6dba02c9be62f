"""fp64 references, fp32 restatements and the one error bound of the training backward kernels (goal_force_amd/csrc/gf_backward.hip).
Plain helper: CPU tensors in, CPU tensors out, no GPU and no project import.

* `*_ref`: the operation in fp64 on the bf16 inputs upcast to fp64, nothing rounded in between.  The two row operations are
  differentiated by fp64 autograd of the FORWARD function, so the reference shares no formula with the kernels.
* `*_f32`: the kernel's own chain written out in fp32 torch (the same formulas, another summation order), result rounded once to bf16
  as the kernel does.  tests/test_backward_refs_cpu.py holds them against the references through the bound — that is the evidence that
  a right kernel passes — and injects faults into them (`fault=`) to show that a subtly wrong one does not.
* `violations` / `assert_within`: for every element  |got - ref| <= 2^-8 |ref| + 2^-16 scale.
    2^-8 |ref|    half a bf16 ulp of the exact value (8 significand bits): what round-to-nearest-even of a right answer costs;
    2^-16 scale   ~128 fp32 epsilons of the quantity's natural magnitude: fp32 evaluation in another summation order.
  `scale` is the rms of the reference row for the row kernels, |df| for act_bwd, |k (pred - target)| for the MSE gradient.
  Neither term is fitted to the code under test, and no element is left out.
"""
import math

import torch

BF = torch.bfloat16
REL = 2.0 ** -8
ABS = 2.0 ** -16
FAULTS = ("mean_drops_last_8", "rope_sin_sign", "scale_for_1p_scale", "dw_after_weight")


# ---------------------------------------------------------------------------------------------------------------------
# the bound
def row_rms(ref):
    """[rows, 1] rms of each reference row: the `scale` of the row kernels."""
    return ref.double().pow(2).mean(-1, keepdim=True).sqrt()


def violations(got, ref, scale):
    """(number of elements outside the bound, worst |got - ref| / allowance, elements) — non-finite `got` counts as outside."""
    got, ref = got.double(), ref.double()
    allow = REL * ref.abs() + ABS * torch.as_tensor(scale, dtype=torch.float64).abs()
    err = (got - ref).abs()
    bad = ~(err <= allow)                                          # NaN / inf in got -> bad
    ratio = torch.where(allow > 0, err / allow, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    ratio = torch.nan_to_num(ratio, nan=math.inf)
    return int(bad.sum()), float(ratio.max()) if ratio.numel() else 0.0, got.numel()


def assert_within(got, ref, scale, what):
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    n, worst, total = violations(got, ref, scale)
    print(f"{what}: {n}/{total} elements outside 2^-8|ref| + 2^-16 scale, worst error {worst:.3f} of the allowance")
    assert n == 0, f"{what}: {n} of {total} elements outside the bound (worst {worst:.2f}x the allowance)"


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def floor_ratio(got, ref):
    """Worst per-row rel-L2 of `got` over the bf16 rounding floor of that row, rel_l2(ref.to(bf16), ref): 1.0 = nothing but the final
    rounding.  Rows whose reference is all zero are skipped."""
    ref, got = ref.double(), got.double()
    fl = (ref.to(BF).double() - ref).norm(dim=-1)
    keep = fl > 0
    return float(((got - ref).norm(dim=-1)[keep] / fl[keep]).max()) if bool(keep.any()) else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# inputs
def rope_table(rows, head_dim, generator, scale=1.0):
    """fp32 (cos, sin) [rows, head_dim/2] of random angles, times `scale` (a table that is not unit-modulus: the q pre-scale)."""
    ang = torch.rand((rows, head_dim // 2), generator=generator, dtype=torch.float64) * (2 * math.pi)
    return (torch.cos(ang) * scale).float().contiguous(), (torch.sin(ang) * scale).float().contiguous()


def row_inputs(rows, dim, generator, gmode="none"):
    """bf16 (x, dy, g) of a row-kernel case.  gmode: 'none' | 'affine' (a weight around 1) | 'scale1p' (bf16(1 + scale))."""
    x = (torch.randn((rows, dim), generator=generator) * 1.5 + 0.3).to(BF)
    dy = torch.randn((rows, dim), generator=generator).to(BF)
    if gmode == "none":
        g = None
    elif gmode == "affine":
        g = (1 + 0.2 * torch.randn((dim,), generator=generator)).to(BF)
    elif gmode == "scale1p":
        g = (1 + (0.3 * torch.randn((dim,), generator=generator)).to(BF).float()).to(BF)
    else:
        raise ValueError(gmode)
    return x, dy, g


ACT_SPECIALS = (0.0, -0.0, 1e-30, -1e-30, 88.0, -88.0, -104.0, 200.0, -200.0, 1e4, -1e4)


def act_inputs(n, generator):
    """bf16 (u, df) of n elements: the special values, a sweep over -30..30, then normal draws x3; the first n of them."""
    sweep = torch.linspace(-30.0, 30.0, 2049)
    u = torch.cat([torch.tensor(ACT_SPECIALS), sweep, 3 * torch.randn((max(n, 8),), generator=generator)])[:n]
    df = torch.randn((n,), generator=generator)
    df[: min(n, 4)] = torch.tensor([1.0, -1.0, 3.0, 0.5])[: min(n, 4)]
    return u.to(BF), df.to(BF)


# ---------------------------------------------------------------------------------------------------------------------
# fp64 references
def layernorm_bwd_ref(x, dy, g=None, eps=1e-6):
    """(dx, dg, db) of y = layer_norm(x, eps) * g + b by fp64 autograd (g None: no multiplier; dg = sum dy xhat, db = sum dy all the same)."""
    dim = x.shape[-1]
    with torch.enable_grad():
        xd = x.double().requires_grad_(True)
        gd = (torch.ones(dim, dtype=torch.float64) if g is None else g.double()).requires_grad_(True)
        bd = torch.zeros(dim, dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.layer_norm(xd, (dim,), None, None, eps) * gd + bd
        y.backward(dy.double())
    return xd.grad, gd.grad, bd.grad


def rope_forward(y, cos, sin, head_dim):
    """Complex rotation of adjacent pairs of every head by the table (cos + i sin)[row, pair]; fp64; differentiable."""
    rows, dim = y.shape
    yc = torch.view_as_complex(y.reshape(rows, dim // head_dim, head_dim // 2, 2))
    yc = yc * torch.complex(cos.double(), sin.double())[:rows, None, :]
    return torch.view_as_real(yc).flatten(1)


def rmsnorm_rope_bwd_ref(x, dy, w, cos=None, sin=None, head_dim=128, eps=1e-6):
    """(dx, dw) of y = rope(x * rsqrt(mean(x^2) + eps) * w) by fp64 autograd; the table may be non-unit-modulus."""
    with torch.enable_grad():
        xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
        y = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps) * wd
        if cos is not None:
            y = rope_forward(y, cos, sin, head_dim)
        y.backward(dy.double())
    return xd.grad, wd.grad


_K0, _K1 = 0.7978845608028654, 0.044715


def act_grad_ref(u, kind):
    """gelu_tanh'(u) | silu'(u) in fp64, closed form."""
    u = u.double()
    if kind == "gelu_tanh":
        t = torch.tanh(_K0 * (u + _K1 * u ** 3))
        return 0.5 * (1 + t) + 0.5 * u * (1 - t * t) * _K0 * (1 + 3 * _K1 * u * u)
    if kind == "silu":
        sg = torch.sigmoid(u)
        return sg * (1 + u * (1 - sg))
    raise ValueError(kind)


def act_bwd_ref(u, df, kind):
    return df.double() * act_grad_ref(u, kind)


def colsum_ref(a, b=None):
    return (a.double() if b is None else a.double() * b.double()).sum(0)


def gated_ref(a, gate):
    """What colsum's `out` must be, bit for bit: one fp32 product rounded once to bf16."""
    return (a.float() * gate.float()).to(BF)


def mse_ref(pred, target, weight):
    """(loss, dpred) = (weight mean(d^2), k d) with d = pred - target, k = 2 weight / n; fp64."""
    d = pred.double() - target.double()
    return weight * float(d.pow(2).mean()), (2.0 * weight / d.numel()) * d


def sumsq_ref(x):
    return float(x.double().pow(2).sum())


def adamw_ref(p, g, m, v, step, lr, betas, eps, weight_decay, grad_scale):
    """One torch.optim.AdamW step (decoupled decay) in fp64 -> (p, m, v):
    p *= 1 - lr wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr/(1-b1^t) m / (sqrt(v)/sqrt(1-b2^t) + eps),  g = grad * grad_scale."""
    b1, b2 = betas
    gr = g.double() * grad_scale
    pd = p.double() * (1 - lr * weight_decay)
    md = b1 * m.double() + (1 - b1) * gr
    vd = b2 * v.double() + (1 - b2) * gr * gr
    denom = vd.sqrt() / math.sqrt(1 - b2 ** step) + eps
    return pd - lr / (1 - b1 ** step) * (md / denom), md, vd


# ---------------------------------------------------------------------------------------------------------------------
# fp32 restatements of the kernels' chains (result rounded once to bf16), with optional injected faults
def _f(t):
    return t.float()


def layernorm_bwd_f32(x, dy, g=None, eps=1e-6, fault=None):
    """layernorm_bwd_kernel / layernorm_bwd_wave_kernel -> (dx bf16, dg fp32, db fp32)."""
    xf, df = _f(x), _f(dy)
    dim = x.shape[-1]
    mean = xf.sum(-1, keepdim=True) / dim
    t = xf - mean
    rstd = 1.0 / torch.sqrt((t * t).sum(-1, keepdim=True) / dim + torch.tensor(eps, dtype=torch.float32))
    xh = t * rstd
    gf = None if g is None else _f(g)
    if fault == "scale_for_1p_scale" and gf is not None:
        gf = gf - 1.0
    dxh = df if gf is None else df * gf
    n = dim - 8 if fault == "mean_drops_last_8" else dim
    m1 = dxh[:, :n].sum(-1, keepdim=True) / dim
    m2 = (dxh * xh)[:, :n].sum(-1, keepdim=True) / dim
    dx = rstd * (dxh - m1 - xh * m2)
    return dx.to(BF), (df * xh).sum(0), df.sum(0)


def rmsnorm_rope_bwd_f32(x, dy, w, cos=None, sin=None, head_dim=128, eps=1e-6, fault=None):
    """rmsnorm_rope_bwd_kernel / rmsnorm_rope_bwd_wave_kernel -> (dx bf16, dw fp32)."""
    xf, dz, wf = _f(x), _f(dy), _f(w)
    rows, dim = x.shape
    if cos is not None:                                            # transpose of [[c, -s], [s, c]] on every pair
        p = dz.reshape(rows, dim // head_dim, head_dim // 2, 2)
        c, s = cos[:rows, None, :], sin[:rows, None, :]
        if fault == "rope_sin_sign":
            s = -s
        dz = torch.stack([p[..., 0] * c + p[..., 1] * s, -p[..., 0] * s + p[..., 1] * c], -1).reshape(rows, dim)
    rstd = 1.0 / torch.sqrt((xf * xf).sum(-1, keepdim=True) / dim + torch.tensor(eps, dtype=torch.float32))
    xn = xf * rstd
    if fault == "dw_after_weight":
        dz = dz * wf
        dw = (dz * xn).sum(0)
    else:
        dw = (dz * xn).sum(0)
        dz = dz * wf
    n = dim - 8 if fault == "mean_drops_last_8" else dim
    m2 = (dz * xn)[:, :n].sum(-1, keepdim=True) / dim
    return (rstd * (dz - xn * m2)).to(BF), dw


def act_bwd_f32(u, df, kind):
    x = _f(u)
    if kind == "gelu_tanh":
        k0, k1 = torch.tensor(_K0, dtype=torch.float32), torch.tensor(_K1, dtype=torch.float32)
        t = torch.tanh(k0 * (x + k1 * x * x * x))
        gr = 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * k0 * (1.0 + 3.0 * k1 * x * x)
    else:
        sg = 1.0 / (1.0 + torch.exp(-x))
        gr = sg * (1.0 + x * (1.0 - sg))
    return (_f(df) * gr).to(BF)


def colsum_f32(a, b=None):
    return (_f(a) if b is None else _f(a) * _f(b)).sum(0)


def mse_f32(pred, target, weight):
    d = _f(pred) - _f(target)
    n = d.numel()
    w = torch.tensor(weight, dtype=torch.float32)
    k = 2.0 * w / torch.tensor(float(n), dtype=torch.float32)
    return float((d * d).sum() * w / torch.tensor(float(n), dtype=torch.float32)), (k * d).to(BF)


def sumsq_f32(x):
    return float((_f(x) * _f(x)).sum())


def adamw_f32(p, g, m, v, step, lr, betas, eps, weight_decay, grad_scale):
    """adamw_kernel -> (p bf16, m fp32, v fp32); every scalar an fp32, as the C ABI receives them."""
    f = lambda s: torch.tensor(s, dtype=torch.float32)            # noqa: E731
    lr_, b1, b2, eps_, wd, gs = (f(s) for s in (lr, betas[0], betas[1], eps, weight_decay, grad_scale))
    bc1 = 1.0 - torch.pow(b1, f(float(step)))
    bc2s = torch.sqrt(1.0 - torch.pow(b2, f(float(step))))
    gr = _f(g) * gs
    pv = (_f(p) * (1.0 - lr_ * wd)).to(BF).float()
    mv = b1 * m + (1.0 - b1) * gr
    vv = b2 * v + (1.0 - b2) * gr * gr
    return (pv - (lr_ / bc1) * (mv / (torch.sqrt(vv) / bc2s + eps_))).to(BF), mv, vv


# ---------------------------------------------------------------------------------------------------------------------
# AdamW: the cases, the state and the bars shared by the CPU and the GPU test
ADAMW_CASES = [dict(step=s, grad_scale=gs, betas=b, eps=e, weight_decay=wd, moments=mo)
               for s, gs, b, e, wd, mo in [(1, 1.0, (0.9, 0.999), 1e-8, 0.1, False), (1, 0.37, (0.9, 0.999), 1e-8, 0.0, False),
                                           (1000, 0.37, (0.8, 0.95), 1e-6, 0.1, True), (1000, 1.0, (0.8, 0.95), 1e-8, 0.0, True),
                                           (1, 0.37, (0.8, 0.95), 1e-6, 0.1, True), (1000, 0.37, (0.9, 0.999), 1e-6, 0.0, False)]]


def adamw_state(n, moments, seed):
    g = torch.Generator().manual_seed(seed)
    p, gr = torch.randn((n,), generator=g).to(BF), torch.randn((n,), generator=g).to(BF)
    m = 0.1 * torch.randn((n,), generator=g) if moments else torch.zeros(n)
    v = (0.1 * torch.randn((n,), generator=g)).pow(2) + 1e-4 if moments else torch.zeros(n)
    return p, gr, m, v


def adamw_check(p, m, v, ref, what):
    """The bars of one AdamW step against the fp64 chain: m 1e-5, v 1e-4 rel-L2 (the kernel forms 1 - beta2 in fp32: 1.3e-5 on v alone);
    the parameter pays two bf16 roundings (the decayed parameter and the result): |p - ref| <= 2^-7 |ref| + 2^-16."""
    p_ref, m_ref, v_ref = ref
    em, ev = rel_l2(m, m_ref), rel_l2(v, v_ref)
    worst = float(((p.double() - p_ref).abs() / (2.0 ** -7 * p_ref.abs() + 2.0 ** -16)).max())
    print(f"{what}: m {em:.2e} v {ev:.2e} p worst {worst:.3f} of the allowance")
    assert em <= 1e-5 and ev <= 1e-4, (what, em, ev)
    assert worst <= 1.0, (what, worst)


def adamw_id(c):
    return "-".join(f"{k}{v}" for k, v in c.items()).replace(" ", "")
