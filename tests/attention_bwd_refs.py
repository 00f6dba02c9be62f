"""fp64 reference, fp32 restatement and the error bounds of the attention backward (goal_force_amd/csrc/gf_attention_bwd.hip).
Plain helper: CPU tensors in, CPU tensors out, no GPU and no project import.  head_dim is 128; q, dout, o, dq are [Sq, heads*128],
k, v, dk, dv [Skv, heads*128], lse [Sq, heads] in the log2 domain.

* `grads_ref`: fp64 autograd of the written-out forward on the bf16 inputs upcast, so it shares no formula with the kernels; with it the
  per-head fp64 intermediates P, dS, delta the bounds are built from.
* `kernel_inputs`: the o and lse the kernels are fed in the isolated tests — the exact o rounded once to bf16, the exact lse2 rounded once
  to fp32: the forward kernels' own error and the plain-q / pre-scaled-q lse mismatch stay out of the backward's bill.
* `chain_f32`: the kernels' chain restated in torch in another summation order (delta from the bf16 o, P = exp2(fma(S, c, -lse)) and dS
  in fp32, ONE bf16 rounding of P for dV = P^T dO, one of dS for dQ and dK, results rounded once), with injected faults (`fault=`).
  tests/test_attention_bwd_refs_cpu.py holds it against the reference through both bounds — the evidence that a right kernel passes — and
  shows that every fault is outside.

THE ELEMENT BOUND, derived and not fitted, with u = 2^-8 (the unit roundoff of bf16), no element left out, non-finite `got` outside:
      |got - ref| <= u |ref| + u W + 2^-16 rms(ref row of the head)
    u |ref|      the one rounding of the result;
    u W          the worst case of the operand roundings and of delta's inherited rounding of o, with D_i = sum_d |dO_id| |O_id|:
                   dq: W[i,d] = scale sum_j (|dS_ij| + P_ij D_i) |K_jd|     dS_ij is rounded once (u |dS_ij|); delta_i = sum dO.bf16(O) is
                   dk: W[j,d] = scale sum_i (|dS_ij| + P_ij D_i) |Q_id|     off by at most u D_i, which moves dS_ij by P_ij u D_i;
                   dv: W[j,d] = sum_i P_ij |dO_id|                          P_ij is rounded once.
                 The delta term is essential: at peaky logits dS = P (dP - delta) is a cancellation, and without it a right chain is
                 outside by orders of magnitude;
    2^-16 rms    ~128 fp32 epsilons of the row's magnitude: fp32 evaluation in another summation order (as tests/backward_refs.py).

THE ROW STATISTIC, for what a worst-case bound cannot see (a second rounding, a 2 % error of one row): the norm of a (row, head)'s 128
deviations from the row's CENTRE over the root-sum-square of the PREDICTED rounding noise.  The centre is the exact gradient GIVEN the
bf16 o the kernels are fed (delta_b = sum dO bf16(o), dS_b = P (dP - delta_b), dq = scale dS_b K, dk = scale dS_b^T Q; dv is the
reference itself): delta's inherited error is a known shift, not noise.  Each rounding is taken as independent and uniform within half
an ulp h(x) of the rounded value (variance h^2 / 3):
      dq: var[i,d] = scale^2 sum_j vS_ij K_jd^2 + h(centre)^2/3 + (2^-16 rms)^2        vS_ij = h(dS_b ij)^2/3 + slop_ij^2
      dk: var[j,d] = scale^2 sum_i vS_ij Q_id^2 + h(centre)^2/3 + (2^-16 rms)^2        slop_ij = 2^-20 P_ij |dO_i| (|V_j| + |O_i|)
      dv: var[j,d] = sum_i h(P_ij)^2/3 dO_id^2  + h(centre)^2/3 + (2^-16 rms)^2
  (slop: the fp32 evaluation of the cancellation dP - delta, ~sqrt(128) fp32 epsilons of the two dot products' magnitude; it is what is
  left where dS is zero in exact math.)  1.0 means "exactly the predicted noise".  The threshold is MEASURED, not chosen: ROW_CHAIN_WORST
  is the worst ratio of chain_f32 (right, no fault) over every case the GPU tests run (all_cases(): the tile-edge pairs at heads 1 and 3,
  the XCD cases, every data class), as tests/test_attention_bwd_refs_cpu.py measures and asserts it; the kernels' bar is ROW_BAR = 1.25 x
  that (summation order and the hardware exp2).  Measured: 1.866 over every class but far_below / far_above, 3.162 over those two; held
  here as 1.9 and 3.2 (the CPU's fp32 matmul order may move the last digits), so the bars are 2.375 and 4.0.  A ratio above 1 on a right
  chain comes from rows whose deviation is ONE random variable: a row with one dominant term (a single uniform rounding reaches
  sqrt(3) of its standard deviation), and in the far_* classes every row of dq and dk — q and k are a
  common vector plus a little noise, sum_j dS_ij = 0 cancels the common part of the result while the roundings of dS_ij all land on it,
  so the row's 128 deviations are one Gaussian sum and the worst of ~500 rows lies near 3 standard deviations.  Those two classes keep
  their own, wider bar so that the others' stays sharp: against bar 2.375 the second rounding of fault `ds_from_rounded_p` measures
  2.7 on dq (2.2 on dk: under the bar; 1.9 at the smaller shape) and a 2 % error of one row 7 - 11.
"""
import math
import types

import torch

BF = torch.bfloat16
HD = 128
U = 2.0 ** -8
ABS = 2.0 ** -16
LOG2E = 1.4426950408889634
ROW_CHAIN_WORST = {"far": 3.2, "rest": 1.9}      # measured: the docstring; tests/test_attention_bwd_refs_cpu.py asserts both figures
ROW_BAR = {k: 1.25 * w for k, w in ROW_CHAIN_WORST.items()}
FAULTS = ("dk_row_5pct", "dq_drops_last_key", "delta_from_row_plus_32", "lse_transposed", "ds_from_rounded_p")


# ---------------------------------------------------------------------------------------------------------------------
# the cases shared by the CPU and the GPU test
Q_LENS = (1, 15, 16, 17, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 255, 256, 257, 289)
KV_LENS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 143, 144, 145, 191, 192, 193, 257, 320, 385)


def _covering_pairs():
    """Two query lengths for every key length, so chosen that every query length meets at least two key lengths as well (3 is a unit
    modulo 19: each of the two series walks through all query lengths)."""
    n = len(Q_LENS)
    out = []
    for i, kv in enumerate(KV_LENS):
        for qi in ((3 * i) % n, (3 * i + 10) % n):
            out.append((Q_LENS[qi], kv))
    return out


TILE_PAIRS = _covering_pairs()                                          # 56 (q_len, kv_len)
TILE_HEADS = (1, 3)
XCD_CASES = [(257, 193, 8), (33, 385, 8), (257, 193, 16), (33, 385, 16)]      # (q_len, kv_len, heads): >= 2 query or key blocks per head
CLASS_SHAPES = [(97, 145), (257, 193)]
CLASS_HEADS = 2
CLASSES = ("std3", "std8", "prescaled", "far_below", "far_above", "dout_zero_rows", "v_const", "delta0")
FAR_BELOW_CONTROL = (97, 192)                                           # kv_len % 64 == 0: no padded key in the dQ kernel's last tile


def all_cases():
    """(class, q_len, kv_len, heads) of every case the GPU tests hold against the bounds."""
    out = [("std1", sq, skv, h) for sq, skv in TILE_PAIRS for h in TILE_HEADS]
    out += [("std1", sq, skv, h) for sq, skv, h in XCD_CASES]
    out += [(c, sq, skv, CLASS_HEADS) for c in CLASSES for sq, skv in CLASS_SHAPES]
    out.append(("far_below", *FAR_BELOW_CONTROL, CLASS_HEADS))
    return out


def case_seed(name, sq, skv, heads):
    return 100003 * sq + 101 * skv + 7 * heads + sum(map(ord, name))


def q_prescale():
    """fp32(fp32(1 / sqrt(128)) x fp32(log2 e)): the factor the forward folds into q when it is handed a pre-scaled q."""
    return float(torch.tensor(1.0 / math.sqrt(HD), dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))


def case_inputs(name, sq, skv, heads, generator):
    """bf16 (q, k, v, dout) and the softmax scale of one data class:
    std1 / std3 / std8   normal data, q and k scaled to that standard deviation of the logits;
    prescaled            the training call: q' = bf16(q c) with c = fp32(log2 e / sqrt 128) and scale = ln 2 (logit std 3);
    far_below            every score far below zero (q ~ 3 u, k ~ -3 u, |u|^2 = 128: lse2 ~ -140), two dout rows zero;
    far_above            every score far above zero (k ~ +3 u: lse2 ~ +150);
    dout_zero_rows       every third row of dout zero;
    v_const              v the same row for every key: dS = 0 in exact math;
    delta0               delta = 0 exactly on every third query: v is zero in the first 64 columns of each head, those rows of dout
                         everywhere else."""
    D = heads * HD
    rn = lambda n: torch.randn((n, D), generator=generator)          # noqa: E731
    q, k, v, dout = rn(sq), rn(skv), rn(skv), rn(sq)
    scale = 1.0 / math.sqrt(HD)
    if name == "std1":
        pass
    elif name in ("std3", "std8"):
        a = math.sqrt(float(name[3:]))
        q, k = q * a, k * a
    elif name == "prescaled":
        q, k = q * math.sqrt(3.0), k * math.sqrt(3.0)
        q, scale = q * q_prescale(), math.log(2.0)
    elif name in ("far_below", "far_above"):
        q, k = 3.0 + 0.1 * q, (-3.0 if name == "far_below" else 3.0) + 0.1 * k
        dout[0] = 0
        dout[min(5, sq - 1)] = 0
    elif name == "dout_zero_rows":
        dout[::3] = 0
    elif name == "v_const":
        v = v[:1].expand(skv, D).clone()
    elif name == "delta0":
        vh, dh = v.view(skv, heads, HD), dout.view(sq, heads, HD)
        vh[:, :, :HD // 2] = 0
        dh[::3, :, HD // 2:] = 0
    else:
        raise ValueError(name)
    return q.to(BF), k.to(BF), v.to(BF), dout.to(BF), scale


def embed(t, rows_after, cols_after, fill=math.nan):
    """A view of t's values inside a larger buffer filled with `fill`: rows_after rows behind it, cols_after columns to its right."""
    big = torch.full((t.shape[0] + rows_after, t.shape[1] + cols_after), fill, dtype=t.dtype, device=t.device)
    big[:t.shape[0], :t.shape[1]] = t
    return big[:t.shape[0], :t.shape[1]]


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 reference
def _heads(t, heads):
    return t.view(t.shape[0], heads, HD).transpose(0, 1)              # [heads, S, 128]


def _flat(t):
    return t.transpose(0, 1).reshape(t.shape[1], -1)                  # [S, heads*128]


def grads_ref(q, k, v, dout, heads, scale):
    """fp64 o, lse2 [Sq, heads], dq, dk, dv by autograd of the written-out forward, and the per-head intermediates P, dS [heads, Sq, Skv],
    delta [heads, Sq] (computed beside it, for the bounds only); the inputs ride along (`ref.q` ...)."""
    with torch.enable_grad():
        qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
        s = scale * (_heads(qd, heads) @ _heads(kd, heads).transpose(1, 2))
        m = s.amax(-1, keepdim=True)
        e = torch.exp(s - m)
        den = e.sum(-1, keepdim=True)
        p = e / den
        o = _flat(p @ _heads(vd, heads))
        o.backward(dout.double())
    p, o = p.detach(), o.detach()
    lse2 = ((m + torch.log(den)).detach().squeeze(-1) * LOG2E).transpose(0, 1).contiguous()
    doh = _heads(dout.double(), heads)
    delta = (doh * _heads(o, heads)).sum(-1)
    ds = p * (doh @ _heads(v.double(), heads).transpose(1, 2) - delta[:, :, None])
    return types.SimpleNamespace(q=q, k=k, v=v, dout=dout, heads=heads, scale=scale, o=o, lse2=lse2, dq=qd.grad, dk=kd.grad, dv=vd.grad,
                                 P=p, dS=ds, delta=delta, _bounds=None)


def kernel_inputs(ref):
    """(o bf16, lse fp32 [Sq, heads] contiguous): the exact values rounded once."""
    return ref.o.to(BF), ref.lse2.float().contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 restatement of the kernels' chain, with optional injected faults
def chain_f32(q, k, v, o, dout, lse, heads, scale, fault=None):
    """attn_bwd_delta16_kernel + attn_bwd_dq16_kernel + attn_bwd_dkv48_kernel -> (dq, dk, dv) bf16.  Faults:
    dk_row_5pct             key row Skv/2 of dK (head 0) 5 % too large;
    dq_drops_last_key       the last key is left out of dQ (a ragged tail's descriptor one row short);
    delta_from_row_plus_32  the queries of granule 0 take their delta from 32 rows further on (a granule record off by one);
    lse_transposed          lse read as [heads, Sq];
    ds_from_rounded_p       dS built from the bf16-rounded P (a second rounding)."""
    assert fault is None or fault in FAULTS, fault
    sq, skv = q.shape[0], k.shape[0]
    qh, kh, vh, oh, doh = (_heads(t.float(), heads) for t in (q, k, v, o, dout))
    delta = (doh * oh).sum(-1)                                                    # [heads, Sq]
    if fault == "delta_from_row_plus_32":
        idx = torch.arange(sq)
        idx[:32] = (idx[:32] + 32).clamp_max(sq - 1)
        delta = delta[:, idx]
    lse = lse.float()
    if fault == "lse_transposed":
        lse = lse.reshape(heads, sq).transpose(0, 1)
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    s = qh @ kh.transpose(1, 2)
    # fma(S, c, -lse): the fp32 product is exact in fp64, so this is the fused result up to a double rounding
    p = torch.exp2((s.double() * c.double() - lse.transpose(0, 1).double()[:, :, None]).float())
    pb = p.to(BF).float()
    ds = (pb if fault == "ds_from_rounded_p" else p) * (doh @ vh.transpose(1, 2) - delta[:, :, None])
    dsb = ds.to(BF).float()
    sc = torch.tensor(scale, dtype=torch.float32)
    dv = pb.transpose(1, 2) @ doh
    dk = (dsb.transpose(1, 2) @ qh) * sc
    dq = ((dsb[:, :, :-1] @ kh[:, :-1]) if fault == "dq_drops_last_key" else (dsb @ kh)) * sc
    if fault == "dk_row_5pct":
        dk[0, skv // 2] *= 1.05
    return tuple(_flat(t).to(BF) for t in (dq, dk, dv))


# ---------------------------------------------------------------------------------------------------------------------
# the bounds
def _half_ulp(x):
    """Half a bf16 ulp at |x| (8 significand bits): 2^(floor(log2 |x|) - 8); 0 at 0."""
    m, e = torch.frexp(x)                                                          # |x| = |m| 2^e, 0.5 <= |m| < 1
    return torch.where(m != 0, torch.ldexp(torch.ones_like(x), e - 9), torch.zeros_like(x))


def bounds(ref):
    """{name: (allowance, row centre, predicted variance)} of dq, dk, dv, each [S, heads*128] fp64 (computed once per reference)."""
    if ref._bounds is not None:
        return ref._bounds
    H, sc = ref.heads, ref.scale
    Q, K, V, DO, O = (_heads(t.double(), H) for t in (ref.q, ref.k, ref.v, ref.dout, ref.o))
    P, dS = ref.P, ref.dS
    D = (DO.abs() * O.abs()).sum(-1)                                               # [H, Sq]
    A = dS.abs() + P * D[:, :, None]
    W = {"dq": sc * (A @ K.abs()), "dk": sc * (A.transpose(1, 2) @ Q.abs()), "dv": P.transpose(1, 2) @ DO.abs()}
    # the row statistic's centre: the exact gradients GIVEN the bf16 o the kernels are fed (delta_b), which is a known shift, not noise
    delta_b = (DO * _heads(ref.o.to(BF).double(), H)).sum(-1)
    dSb = P * (DO @ V.transpose(1, 2) - delta_b[:, :, None])
    C = {"dq": sc * (dSb @ K), "dk": sc * (dSb.transpose(1, 2) @ Q), "dv": _heads(ref.dv, H)}
    # fp32 evaluation of the cancellation dP - delta: ~sqrt(128) fp32 epsilons (2^-20) of the two dot products' magnitude
    nDO = DO.norm(dim=-1)
    slop = 2.0 ** -20 * P * (nDO[:, :, None] * V.norm(dim=-1)[:, None, :] + (nDO * O.norm(dim=-1))[:, :, None])
    vS, vP = _half_ulp(dSb) ** 2 / 3 + slop ** 2, _half_ulp(P) ** 2 / 3
    Var = {"dq": sc ** 2 * (vS @ K ** 2), "dk": sc ** 2 * (vS.transpose(1, 2) @ Q ** 2), "dv": vP.transpose(1, 2) @ DO ** 2}
    out = {}
    for n in ("dq", "dk", "dv"):
        r = _heads(getattr(ref, n), H)
        rms = r.pow(2).mean(-1, keepdim=True).sqrt()
        crms = C[n].pow(2).mean(-1, keepdim=True).sqrt()
        out[n] = (_flat(U * r.abs() + U * W[n] + ABS * rms), _flat(C[n]), _flat(Var[n] + _half_ulp(C[n]) ** 2 / 3 + (ABS * crms) ** 2))
    ref._bounds = out
    return out


def measure(got, ref, name):
    """(elements outside the element bound, worst |got - ref| / allowance, worst row ratio) of one gradient; non-finite -> outside / inf."""
    want = getattr(ref, name)
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    allow, centre, var = bounds(ref)[name]
    err = (got.double() - want).abs()
    bad = ~(err <= allow)
    inf, zero = torch.full_like(err, math.inf), torch.zeros_like(err)
    ratio = torch.nan_to_num(torch.where(allow > 0, err / allow, torch.where(err > 0, inf, zero)), nan=math.inf, posinf=math.inf)
    e2, s2 = (t.view(t.shape[0], ref.heads, HD).sum(-1) for t in ((got.double() - centre) ** 2, var))
    row = torch.nan_to_num(torch.where(s2 > 0, (e2 / s2).sqrt(), torch.where(e2 > 0, inf[:, :ref.heads], zero[:, :ref.heads])), nan=math.inf, posinf=math.inf)
    return int(bad.sum()), float(ratio.max()), float(row.max())


def row_bar(data_class):
    return ROW_BAR["far" if data_class.startswith("far_") else "rest"]


def assert_within(got3, ref, what, data_class="std1"):
    """dq, dk, dv against both bounds (the row bar is the data class's); prints what it measures and returns (worst element ratio,
    worst row ratio)."""
    bar = row_bar(data_class)
    worst_e = worst_r = 0.0
    fails = []
    for name, got in zip(("dq", "dk", "dv"), got3):
        n, we, wr = measure(got, ref, name)
        print(f"{what} {name}: {n}/{got.numel()} elements outside u|ref| + uW + 2^-16 rms, worst error {we:.3f} of the allowance; "
              f"worst row {wr:.3f} x the predicted noise (bar {bar:.3f})")
        if n:
            fails.append(f"{name}: {n} of {got.numel()} elements outside the bound (worst {we:.2f}x the allowance)")
        if not wr <= bar:
            fails.append(f"{name}: a row's error is {wr:.2f}x the predicted rounding noise (bar {bar:.3f})")
        worst_e, worst_r = max(worst_e, we), max(worst_r, wr)
    assert not fails, f"{what}: " + "; ".join(fails)
    return worst_e, worst_r


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
