"""The exact chains, fp32 restatements and bars of the VAE kernels: the five convolution kernels (gf_vae_im2col + gf_gemm_bf16, the two
gathers of gf_conv3d_bf16 = gemm_ph_kernel<CONV = 1, 2>, the direct 96-channel and the direct upsample kernel of gf_conv_direct.hip,
gf_conv3d_padded_bf16) and the row kernels of gf_vae.hip (gf_vae_rmsnorm_silu, gf_softmax_rows, gf_vae_prep_latent,
gf_vae_finish_latent).  Plain helper: CPU tensors in, CPU tensors out, no GPU and no project import.

Layout: activations are channels-last [T, H, W, C] bf16 as the kernels take them; `hist` is the two cached frames [2, H, W, C] (None =
zeros = no history); w is [N, >= kt ks ks C] with the header's column order (dt, dy, dx, cin).

CONVOLUTION
* `conv_reference(x, hist, w, bias, kt, ks, mode, t_stride, t_off, t_out, resid=None)` -> (acc, S), both [t_out Ho Wo, N] fp64.  Written
  from include/goalforce.h and the reference's CausalConv3d / Resample (VAE:33-52, 82-174) with torch's own F.conv3d in fp64 on NCDHW
  tensors — no patch matrix of its own:
      kt = 3: the two history frames are concatenated IN FRONT in time (frame -2, frame -1, x);
      mode 0: zero padding ks // 2;   mode 1: repeat_interleave(2) in H and W, then padding 1;   mode 2: F.pad(.., (0, 1, 0, 1)), stride 2;
      output frame j is the convolution whose LAST temporal tap is input frame t_off + j t_stride (causal: taps reach kt - 1 back);
      the weight is w[:, :kt ks ks C] reshaped (N, kt, ks, ks, C) -> [N, C, kt, ks, ks].
  S is the same convolution of |x| and |w|.  bias and resid take no part (they are the chain's); the arguments are there so that a
  case's dict can be splatted.
* The chain is gemm_refs.chain(acc, bias, EPI_BIAS | EPI_RESID, resid, None, S=S):  bf16(acc + bias)  |  bf16(resid + bf16(acc + bias)),
  and the bars are gemm_refs.judge's, unchanged (derived there, not fitted):
      (a) differing bf16 bits on at most 2^-10 of the output, per row and column at most the binomial cap;
      (b) every element within 2^-7 m + L K 2^-23 S, K = kt ks ks C products per output, L = 1.
  gemm_refs limits its random cases to K <= 1024 out of caution about (a) (a stage flips with probability ~sqrt(K) 2^-15).  The VAE's
  convolutions have K up to 10368; tests/test_vae_refs_cpu.py shows that the fp32 restatement below is inside both bars on every
  Gaussian input the GPU test uses (the premise is on the inputs, not on the kernels), so the caps stay as they are.
* Three data classes (`conv_inputs`):
      selector  weight row n holds a single +-2^k (k in -1, 0, 1) at one (dt, dy, dx, c); the rows cycle through all taps; bias zero;
                activations, history and residual are random bf16 bit patterns with exponents in gemm_refs.BAND.  Every output is
                exactly one shifted input element times a power of two, or zero at a border; resid + that spans 2^4 .. 2^-11, exact in
                fp32 before its rounding.  torch.equal; `selector_explain` names the tap and the border of a differing element.
      integers  activations -4 .. 4, weights -2 .. 2, integer bias and residual -8 .. 8: |acc| <= 8 x 10368 < 2^24, exact in fp32 in
                every order; bf16(acc + bias) and bf16(resid + y) round exact values.  torch.equal, both epilogues.  Carries the geometry.
      gauss     activations 0.7 N(0, 1), weights N(0, 1) / sqrt(K), bias and residual N(0, 1): the two bars.  Carries the rounding
                points and the accumulation.  Below gemm_refs.SMALL outputs the data are drawn again until the restatement gives the
                chain's bits in K tiles of 32 and 64, and below 1024 outputs — where (a) asks for equal bits — until every
                pre-rounding value is clear of the bf16 rounding boundaries as well (`_clear_of_boundaries`).
* `conv_f32(d, epi, ktile, fault)`: the restatement — a host `unfold` of the plainly padded tensor (`patches`), gemm_refs.sum_f32 in the
  kernels' K order (tiles of `ktile` columns of (dt, dy, dx, c)), the epilogue in fp32 torch.  `fault=` is one of CONV_FAULTS.

ROW KERNELS
* `rmsnorm_silu_chain(x, gamma, silu)` (RMS_norm, VAE:55-70: F.normalize(x, dim=C) * sqrt(C) * gamma, every eager op rounding to bf16):
      n = max(bf16(sqrt(sum x^2)), 1e-12);  y1 = bf16(x / n);  y2 = bf16(fp32(y1 fp32(sqrt C)));  y3 = bf16(y2 gamma);  [bf16(silu(y3))]
  in fp64.  x / n is a quotient of two bf16 values and y2 gamma a 16-bit product: both exact before their rounding in fp32 too, and
  y1 sqrt(C) is rounded to fp32 first because the eager multiply by a Python float does that.  The kernel multiplies by a correctly
  rounded 1 / n and claims the result equals the division after rounding, so the chain DIVIDES.  The only order-dependent value is
  the fp32 sum of squares: `rms_inputs` draws every row so that fp64 sqrt(sum x^2) lies at least 2^-14 (relative) from a bf16 rounding
  boundary (a row is drawn again otherwise).  An fp32 sum of C <= 512 non-negative terms is within C 2^-24 <= 2^-15 of the exact sum
  in any order, its root within 2^-16 + 2^-24, so n is the same bf16 value in every summation order and silu = False is torch.equal —
  no element is left out.  silu = True: a function of one bf16 value; held to forward_refs.assert_act on the kernel's own
  silu = False output (at most one bf16 step from bf16(fp64 SiLU), differing share <= 2^-10) and to the same share against the chain.
* `softmax_rows_chain(x, scale, bias, nvalid, ldo)` -> (p, bound), fp64 [rows, ldo]:  a = x scale (exact in fp64: 8 x 24 bits), with a
  bias a = bf16(a + bias);  p = softmax over the first nvalid columns, exactly zero from nvalid to ldo.  The kernel evaluates
  bf16(expf(a_c - mx) (1 / sum_j expf(a_j - mx))) in fp32.  Per element, with u = 2^-24 (half an fp32 ulp, relative):
      the exponent's argument:  fl(x scale) is off by u |a_c| (nothing with a bias: `softmax_inputs` keeps x scale + bias exact in
          fp32, so the rounded sum is the same bf16 value), fl(a_c - mx) by u |a_c - mx|, and the maximum by u |mx| (it cancels between
          numerator and row sum, but is kept):  d_c = u (|a_c| + |mx| + |a_c - mx|), a relative error e^d - 1 <= 1.01 d of the term;
      expf: at most 2 ulp = 4 u (the device's expf is documented at 1 ulp);
      the row sum of nvalid non-negative terms, in any order: (nvalid - 1) u relative, on top of its terms' own errors
          max_j (1.01 d_j + 4 u);  the reciprocal and the product: 2 u more.
      r = 1.01 (d_c + max_j d_j) + (8 + 2 + nvalid) u  bounds the relative error of the fp32 quotient, and the final rounding adds half a
      bf16 spacing of it, at most 2^-8 of the value (not 2^-9: the spacing is relative to the binade's lower end):
          |got - p| <= 2^-8 p (1 + r) + r p + 2^-126,
      the last term for fp32's underflow (expf of an argument below -87 may be flushed; a bf16 output below 2^-126 is denormal).
      This is the derivation of attention_fwd_refs.py's lse bound (argument error, exp, sum) carried to the probability.  Derived, not
      fitted: at scores of std 50 d is 5e-5 against the rounding's 3.9e-3.
* `prep_latent_ref`, `finish_latent_ref`: the header's two-rounding formulas in fp32 torch, bf16(bf16(z / inv_std) + mean) and
  bf16(bf16(x - mean) inv_std): each operation is a single IEEE fp32 operation, so the result is bit for bit what a right kernel gives.
"""
import math

import torch
import torch.nn.functional as F

import gemm_refs as R
from forward_refs import act_ref, bits, rb

BF = torch.bfloat16
CONV_FAULTS = ("mode2_pad_top_left", "hist_swapped", "taps_reversed", "border_wrap", "t_off_plus1", "upsample_round_up",
               "drop_last_32ch", "resid_before_rounding", "patch_row_2pct")
RMS_FAULTS = ("norm_not_rounded", "scale_before_rounding")
SOFTMAX_FAULTS = ("max_over_ncols", "bias_without_rounding")
EPIS = (R.EPI_BIAS, R.EPI_RESID)


def out_hw(H, W, mode):
    return (2 * H, 2 * W) if mode == 1 else ((H // 2, W // 2) if mode == 2 else (H, W))


def frames_read(kt, t_stride, t_off, t_out):
    """The source frames (negative: history) some output frame's window holds."""
    return sorted({t_off + j * t_stride - (kt - 1) + dt for j in range(t_out) for dt in range(kt)})


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 convolution
def _ncdhw(x, hist, kt, t_stride, t_off, t_out):
    """[1, C, frames, H, W] fp64 of exactly the frames the window spans: (history, x)[first tap of output 0 .. last tap of the last]."""
    xd = x.double()
    if kt == 3:
        h = torch.zeros((2,) + tuple(x.shape[1:]), dtype=torch.float64) if hist is None else hist.double()
        xd = torch.cat([h, xd], 0)                                   # frame f of x is now frame f + 2
    first = t_off                                                    # kt = 3: t_off - 2 + 2
    last = t_off + (t_out - 1) * t_stride + kt - 1
    return xd[first:last + 1].permute(3, 0, 1, 2)[None]


def _conv64(xn, wn, ks, mode, t_stride):
    if mode == 1:
        xn = F.pad(xn.repeat_interleave(2, 3).repeat_interleave(2, 4), (1, 1, 1, 1))
        s = 1
    elif mode == 2:
        xn, s = F.pad(xn, (0, 1, 0, 1)), 2
    else:
        p = ks // 2
        xn, s = F.pad(xn, (p, p, p, p)), 1
    return F.conv3d(xn, wn, stride=(t_stride, s, s))


def conv_reference(x, hist, w, bias, kt, ks, mode, t_stride, t_off, t_out, resid=None):
    T, H, W, C = x.shape
    N, k = w.shape[0], kt * ks * ks * C
    assert t_off + (t_out - 1) * t_stride < T and mode in (0, 1, 2) and (mode == 0 or ks == 3)
    xn = _ncdhw(x, hist, kt, t_stride, t_off, t_out)
    wn = w[:, :k].double().reshape(N, kt, ks, ks, C).permute(0, 4, 1, 2, 3).contiguous()
    acc = _conv64(xn, wn, ks, mode, t_stride)
    S = _conv64(xn.abs(), wn.abs(), ks, mode, t_stride)
    Ho, Wo = out_hw(H, W, mode)
    assert tuple(acc.shape) == (1, N, t_out, Ho, Wo), (acc.shape, (N, t_out, Ho, Wo))
    f = lambda t: t[0].permute(1, 2, 3, 0).reshape(t_out * Ho * Wo, N).contiguous()      # noqa: E731
    return f(acc), f(S)


GEOM = ("kt", "ks", "mode", "t_stride", "t_off", "t_out")


def conv_ref(d, epi):
    """The gemm_refs.Ref of a case dict (conv_inputs) under one epilogue; the fp64 convolution is computed once per dict."""
    if "_acc" not in d:
        d["_acc"], d["_S"] = conv_reference(d["x"], d["hist"], d["w"], d["bias"], *(d[k] for k in GEOM))
    return R.Ref(*R.chain(d["_acc"], d["bias"], epi, d["resid"] if epi == R.EPI_RESID else None, None, S=d["_S"]), None, None)


def conv_k(d):
    return d["kt"] * d["ks"] * d["ks"] * d["x"].shape[3]


# ---------------------------------------------------------------------------------------------------------------------
# the three data classes
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def selector_col(n, taps, C):
    """(tap, channel) of weight row n: the rows cycle through the taps, the channel moves on with every round."""
    return n % taps, (n + 5 * (n // taps)) % C


def conv_inputs(cls, T, H, W, C, N, kt, ks, mode=0, t_stride=1, t_off=0, t_out=None, hist=True, kpad=None, seed=0):
    """A case dict: x [T, H, W, C], hist [2, H, W, C] (kt = 3 and `hist`) or None, w [N, kpad] (zero from kt ks ks C), bias [N],
    resid [rows, N], all bf16, and the geometry.  kpad defaults to kt ks ks C rounded up to 64."""
    t_out = (T - t_off + t_stride - 1) // t_stride if t_out is None else t_out
    taps, k = kt * ks * ks, kt * ks * ks * C
    kpad = -(-k // 64) * 64 if kpad is None else kpad
    Ho, Wo = out_hw(H, W, mode)
    rows = t_out * Ho * Wo
    geom = dict(kt=kt, ks=ks, mode=mode, t_stride=t_stride, t_off=t_off, t_out=t_out, cls=cls,
                shape=(T, H, W, C, N), what=f"T{T} H{H} W{W} C{C} N{N} kt{kt} ks{ks} mode{mode} ts{t_stride} off{t_off} out{t_out}")
    want_hist = kt == 3 and hist
    for attempt in range(512):
        g = _gen(9176 * seed + 131 * attempt + 7919 * T + 31 * H + 17 * W + 3 * C + N + 1000 * kt + 100 * ks + 10 * mode + t_off)
        w = torch.zeros((N, kpad))
        if cls == "selector":
            x = R._band_bf16((T, H, W, C), g)
            h = R._band_bf16((2, H, W, C), g) if want_hist else None
            for n in range(N):
                tap, c = selector_col(n, taps, C)
                w[n, tap * C + c] = (-1.0) ** n * 2.0 ** (n % 3 - 1)
            bias, resid = torch.zeros(N).to(BF), R._band_bf16((rows, N), g)
        elif cls == "integers":
            x = torch.randint(-4, 5, (T, H, W, C), generator=g).to(BF)
            h = torch.randint(-4, 5, (2, H, W, C), generator=g).to(BF) if want_hist else None
            w[:, :k] = torch.randint(-2, 3, (N, k), generator=g).float()
            bias = torch.randint(-8, 9, (N,), generator=g).to(BF)
            resid = torch.randint(-8, 9, (rows, N), generator=g).to(BF)
        else:
            assert cls == "gauss", cls
            x = (0.7 * torch.randn((T, H, W, C), generator=g)).to(BF)
            h = (0.7 * torch.randn((2, H, W, C), generator=g)).to(BF) if want_hist else None
            w[:, :k] = torch.randn((N, k), generator=g) / math.sqrt(k)
            bias = torch.randn(N, generator=g).to(BF)
            resid = torch.randn((rows, N), generator=g).to(BF)
        d = dict(geom, x=x, hist=h, w=w.to(BF), bias=bias, resid=resid)
        if cls != "gauss" or rows * N >= R.SMALL or ((rows * N * R.SHARE_CAP >= 1 or _clear_of_boundaries(d)) and _order_proof(d)):
            return d
    raise RuntimeError(f"conv_inputs({geom['what']}): no draw is clear of the rounding boundaries")


def _order_proof(d):
    for epi in EPIS:
        want = bits(conv_ref(d, epi).out)
        for ktile in (32, 64):
            if not torch.equal(bits(conv_f32(d, epi, ktile)), want):
                return False
    return True


def _clear_of_boundaries(d):
    """Outputs of fewer than 1024 elements, where bar (a) asks for equal bits: every pre-rounding value acc + bias lies at least
    2^-17 max(|acc + bias|, Q) from a bf16 rounding boundary, Q = sqrt(sum (x w)^2) the size of the walk the partial sums take.  A right
    kernel's accumulator is off by the roundings of its K / 32 + 1 fp32 additions (one per 32-channel MFMA and the bias), each at most
    2^-24 of a partial sum of size ~Q: sqrt(K / 32) 2^-24 Q <= 2^-19.8 Q at K = 10368, so the margin is more than seven of its standard
    deviations in any order (a value that cancels to near zero included, where the spacing of bf16 is finer than that error).  A
    condition on the inputs, read off the fp64 reference alone."""
    ref = conv_ref(d, R.EPI_BIAS)
    xn = _ncdhw(d["x"], d["hist"], d["kt"], d["t_stride"], d["t_off"], d["t_out"])
    T, H, W, C, N = d["shape"]
    k = conv_k(d)
    wn = d["w"][:, :k].double().reshape(N, d["kt"], d["ks"], d["ks"], C).permute(0, 4, 1, 2, 3).contiguous()
    Q = torch.sqrt(_conv64(xn ** 2, wn ** 2, d["ks"], d["mode"], d["t_stride"]))[0].permute(1, 2, 3, 0).reshape(-1, N)
    lin = (d["_acc"] + d["bias"].double()).abs()
    e = torch.floor(torch.log2(lin.clamp_min(2.0 ** -126)))
    ulp = torch.exp2(e - 7)
    frac = lin / ulp
    dist = ((frac - torch.floor(frac)) - 0.5).abs() * ulp
    assert ref.out.shape == lin.shape
    return bool((dist >= 2.0 ** -17 * torch.maximum(lin, Q)).all())


def selector_explain(d, row, n):
    """Which tap weight row n selects, which output pixel `row` is, and what that tap reads there."""
    T, H, W, C, _ = d["shape"]
    kt, ks, mode = d["kt"], d["ks"], d["mode"]
    tap, c = selector_col(n, kt * ks * ks, C)
    dt, dy, dx = tap // (ks * ks), tap // ks % ks, tap % ks
    Ho, Wo = out_hw(H, W, mode)
    j, Y, X = row // (Ho * Wo), row // Wo % Ho, row % Wo
    f = d["t_off"] + j * d["t_stride"] - (kt - 1) + dt
    if mode == 2:
        sy, sx, inside = 2 * Y + dy, 2 * X + dx, 2 * Y + dy < H and 2 * X + dx < W
    else:
        yy, xx = Y + dy - ks // 2, X + dx - ks // 2
        inside = 0 <= yy < Ho and 0 <= xx < Wo
        sy, sx = (yy >> 1, xx >> 1) if mode == 1 else (yy, xx)
    src = "the zero border" if not inside else (f"history frame {f}" if f < 0 else f"frame {f}") + f" pixel ({sy}, {sx})"
    return f"output (frame {j}, y {Y}, x {X}) column {n}: tap (dt {dt}, dy {dy}, dx {dx}) channel {c} reads {src}"


# ---------------------------------------------------------------------------------------------------------------------
# the patch matrix by `unfold` of the plainly padded tensor, and the fp32 restatement with its faults
def patches(x, hist, kt, ks, mode, t_stride, t_off, t_out, fault=None):
    """[t_out Ho Wo, kt ks ks C] in x's dtype: column ((dt ks + dy) ks + dx) C + c."""
    T, H, W, C = x.shape
    if fault == "t_off_plus1":
        t_off = t_off + 1 if t_off + 1 + (t_out - 1) * t_stride < T else t_off - 1
    seq = x
    if kt == 3:
        h = torch.zeros((2, H, W, C), dtype=x.dtype) if hist is None else hist
        if fault == "hist_swapped":
            h = h.flip(0)
        seq = torch.cat([h, x], 0)
        if fault == "taps_reversed":                                  # the window starts AT its frame and reads the future
            seq = torch.cat([x, torch.zeros((2, H, W, C), dtype=x.dtype)], 0)
    # with the history in front, frame f of x is frame f + 2: the window of output 0 starts at t_off either way
    seq = seq[t_off:t_off + (t_out - 1) * t_stride + kt].permute(3, 0, 1, 2)       # [C, frames, H, W]
    if mode == 1:
        if fault == "upsample_round_up":                               # source (y + 1) >> 1 instead of y >> 1
            iy = ((torch.arange(2 * H) + 1) >> 1).clamp_max(H - 1)
            ix = ((torch.arange(2 * W) + 1) >> 1).clamp_max(W - 1)
            seq = seq[:, :, iy][:, :, :, ix]
        else:
            seq = seq.repeat_interleave(2, 2).repeat_interleave(2, 3)
        seq, s = F.pad(seq, (1, 1, 1, 1)), 1
    elif mode == 2:
        seq, s = F.pad(seq, (1, 0, 1, 0) if fault == "mode2_pad_top_left" else (0, 1, 0, 1)), 2
    else:
        p = ks // 2
        seq, s = F.pad(seq, (p, p, p, p)), 1
    Ho, Wo = out_hw(H, W, mode)
    win = seq.unfold(1, kt, t_stride).unfold(2, ks, s).unfold(3, ks, s)            # [C, t_out, Ho, Wo, kt, ks, ks]
    assert tuple(win.shape[1:4]) == (t_out, Ho, Wo), (win.shape, t_out, Ho, Wo)
    win = win.permute(1, 2, 3, 4, 5, 6, 0).contiguous()                               # [t_out, Ho, Wo, kt, ks, ks, C]
    if fault == "border_wrap" and mode == 0 and ks == 3 and W > 1:
        # the flat-index error: tap (y, -1) reads (y - 1, W - 1), tap (y, W) reads (y + 1, 0) — the neighbouring image row
        flat = F.pad(seq[:, :, 1:H + 1, 1:W + 1].reshape(C, -1, H * W), (W + 1, W + 1))
        fw = flat.unfold(1, kt, t_stride)                                             # [C, t_out, HW + 2W + 2, kt]
        for dy in range(3):
            for dx in (0, 2):
                sh = (dy - 1) * W + (dx - 1)
                v = fw[:, :, W + 1 + sh:W + 1 + sh + H * W]                           # [C, t_out, HW, kt]
                win[:, :, :, :, dy, dx, :] = v.reshape(C, t_out, H, W, kt).permute(1, 2, 3, 4, 0)
    if fault == "drop_last_32ch":
        win[:, :, :, kt // 2, ks // 2, ks // 2, -min(32, C):] = 0
    return win.reshape(t_out * Ho * Wo, kt * ks * ks * C)


def conv_f32(d, epi, ktile=64, fault=None, order=0):
    """-> bf16 [rows, N]: the patch matrix, the fp32 sum in K tiles of `ktile` (gemm_refs.sum_f32), the epilogue in fp32."""
    a = patches(d["x"], d["hist"], *(d[k] for k in GEOM), fault=fault)
    k = a.shape[1]
    kp = -(-k // ktile) * ktile
    a = F.pad(a.float(), (0, kp - k))
    w = F.pad(d["w"][:, :k].float(), (0, kp - k))
    acc = R.sum_f32(a, w, ktile, order)
    if fault == "patch_row_2pct":                                     # one 8 x 32 output patch: its image row 3 (or the last)
        T, H, W, C, _ = d["shape"]
        Ho, Wo = out_hw(H, W, d["mode"])
        y = min(3, Ho - 1)
        acc[y * Wo:y * Wo + min(32, Wo)] *= 1.02
    lin = acc + d["bias"].float()
    if epi == R.EPI_BIAS:
        return lin.to(BF)
    if fault == "resid_before_rounding":
        return (d["resid"].float() + lin).to(BF)
    return (d["resid"].float() + rb(lin)).to(BF)


def old_bars(got, ref):
    """The whole-tensor bars tests/test_vae.py holds its row kernels to: (rel-L2 < 3e-3, share more than one bf16 step off < 5e-3)."""
    g, r = got.double(), ref.double()
    e = float((g - r).norm() / r.norm().clamp_min(1e-30))
    frac = float((R.bf16_steps(got.to(BF), ref.to(BF)) > 1).double().mean())
    return e < 3e-3, frac < 5e-3, e, frac


# ---------------------------------------------------------------------------------------------------------------------
# the cases both test files walk.  route: how the GPU test reaches the kernel —
#   "general"  gemm_ph_kernel<CONV = 1>: a separate cache (kt = 3), modes 1 and 2, or conv_gather = 1;   "ptr"  <CONV = 2>: the history in
#   front of src (kt = 3) or kt = 1, mode 0;  both with conv_direct = 0;   "c96" / "up": the direct kernels;  "padded": gf_conv3d_padded_bf16.
def _c(route, T, H, W, C, N, kt, ks, **kw):
    return dict(route=route, T=T, H=H, W=W, C=C, N=N, kt=kt, ks=ks, **kw)


# output rows 1, 255, 256, 257, 513 around the 256-row tile; N 8 .. 384 over the 128-, 192- and 256-wide column tiles, full and ragged;
# C 8, 24, 64, 192 (c64 and its complement) and 96 with conv_direct = 0; K with and without padding columns; one K tile; images one
# pixel wide and one pixel tall; t_off > 0; the encoder's strided time convolution
IMPLICIT_CASES = [
    _c("general", 1, 1, 1, 8, 8, 3, 3),                                            # one row; K 216 -> 256
    _c("general", 1, 16, 16, 8, 16, 1, 1),                                         # 256 rows, ONE K tile (K 8 -> 64), conv_gather = 1
    _c("ptr", 1, 1, 257, 24, 96, 1, 3),                                            # one pixel tall, 257 rows
    _c("ptr", 4, 171, 1, 64, 128, 3, 3, t_off=1, t_out=3),                         # one pixel wide, 513 rows, c64, t_off > 0
    _c("general", 1, 8, 8, 64, 136, 1, 3, mode=1),                                 # upsample gather, 256 rows, c64
    _c("general", 2, 30, 34, 24, 192, 1, 3, mode=2, t_off=1, t_out=1),             # stride-2 gather, 255 rows, one 192-wide tile
    _c("general", 6, 9, 19, 192, 200, 3, 1, t_stride=2, t_off=1, t_out=3),         # the encoder's time conv, 513 rows, ragged 256-wide tile
    _c("ptr", 3, 257, 1, 64, 264, 3, 1, t_off=2, t_out=1),                         # decoder time conv, one frame; 257 rows
    _c("ptr", 1, 15, 17, 192, 384, 3, 3),                                          # 255 rows, two 192-wide tiles, K 5184
    _c("general", 3, 9, 19, 24, 200, 3, 3),                                        # separate cache, 513 rows, K 648 -> 704
    _c("ptr", 1, 16, 16, 8, 264, 1, 3),                                            # K 72 -> 128, ragged second 256-wide tile
    _c("ptr", 1, 1, 257, 96, 96, 3, 3),                                            # C = 96 kept on this kernel, K 2592 -> 2624
    _c("ptr", 1, 15, 17, 64, 8, 1, 1, kpad=128),                                   # C % 64 == 0 but K padded: the complement of c64
    _c("general", 3, 9, 19, 64, 128, 3, 3, hist=False),                            # a zero cache = no history; conv_gather irrelevant
]
# workgroup patches of 8 x 32 pixels walking the frames: H 1 .. 17, W 1 .. 65, T_out 1 .. 9 (one / several segments, a shorter last
# one at 5), N = 96 and the RGB head's widths (the ABI takes multiples of 8: 8 and 16), t_off 0 / 2; then the fall-backs (N = 24;
# ldc = N + 8 is the GPU test's)
C96_CASES = [
    _c("c96", 1, 1, 1, 96, 96, 3, 3),
    _c("c96", 4, 7, 31, 96, 8, 3, 3, t_off=2, t_out=2),
    _c("c96", 3, 8, 32, 96, 96, 3, 3),
    _c("c96", 6, 9, 33, 96, 16, 3, 3, t_off=2, t_out=4),
    _c("c96", 5, 17, 65, 96, 8, 3, 3),
    _c("c96", 9, 8, 33, 96, 96, 3, 3),
    _c("c96", 1, 17, 1, 96, 96, 3, 3),
    _c("c96", 2, 1, 65, 96, 96, 3, 3, hist=False),
    _c("c96", 2, 9, 33, 96, 24, 3, 3),                                             # falls back to the implicit GEMM
]
# the 192 -> 96 upsample kernel: Hs 4 / 8 / 12 x Ws 16 / 32 / 48 (one and three output patches each way), T_out 1 .. 4, t_off 0 / 1,
# and the neighbours that fall back (Hs % 4, Ws % 16)
UP_CASES = [
    _c("up", 1, 4, 16, 192, 96, 1, 3, mode=1),
    _c("up", 3, 8, 32, 192, 96, 1, 3, mode=1, t_off=1, t_out=2),
    _c("up", 2, 12, 48, 192, 96, 1, 3, mode=1, t_off=1, t_out=1),
    _c("up", 3, 4, 48, 192, 96, 1, 3, mode=1),
    _c("up", 4, 12, 16, 192, 96, 1, 3, mode=1),
    _c("up", 1, 6, 16, 192, 96, 1, 3, mode=1),
    _c("up", 1, 4, 24, 192, 96, 1, 3, mode=1),
]
# padded row counts (kt - 1 + T)(H + 2)(W + 2) around the 256-row tile: (1, 1, 1); (1, 14, 14) = 256 at kt = 1; (1, 14, 15); (2, 9, 13);
# (3, 6, 30) = 768 at kt = 1.  fill: how the GPU test writes the interior ("copy", "rms" = gf_vae_rmsnorm_silu_padded, "up" =
# gf_vae_upsample2x_padded from a half-size x)
PADDED_CASES = [
    _c("padded", 1, 1, 1, 192, 96, 3, 3),
    _c("padded", 1, 14, 14, 384, 192, 1, 3, hist=False, fill="up"),
    _c("padded", 1, 14, 15, 192, 200, 1, 3, hist=False),
    _c("padded", 2, 9, 13, 384, 384, 3, 3, fill="rms"),
    _c("padded", 3, 6, 30, 192, 96, 1, 3, hist=False),
    _c("padded", 3, 6, 30, 192, 192, 3, 3),
]
FLOP_CAP = 2.5e9        # per fp64 reference (acc and S are one each)


def _flops(c):
    Ho, Wo = out_hw(c["H"], c["W"], c.get("mode", 0))
    t_out = c.get("t_out", (c["T"] - c.get("t_off", 0) + c.get("t_stride", 1) - 1) // c.get("t_stride", 1))
    return 2.0 * t_out * Ho * Wo * c["N"] * c["kt"] * c["ks"] * c["ks"] * c["C"]


def _grids():
    """The axes the issue names, crossed where the hand-made lists above only cover them: every row count against every N on both
    gathers (C and the kernel taking turns), every H against every W of the direct kernel, every Hs against every Ws of the upsample
    kernel, every padded shape against every N.  A combination above FLOP_CAP takes the next cheaper (C, kernel)."""
    imp, c96, up, pad = [], [], [], []
    shapes = {1: (1, 1), 255: (15, 17), 256: (16, 16), 257: (257, 1), 513: (27, 19)}
    kinds = [(8, 1, 3), (24, 3, 3), (64, 3, 1), (192, 1, 1), (192, 3, 3), (64, 1, 3), (24, 3, 1), (8, 3, 3)]
    i = 0
    for rows, (H, W) in shapes.items():
        for N in (8, 96, 128, 136, 192, 200, 264, 384):
            for shift in range(len(kinds)):
                C, kt, ks = kinds[(i + shift) % len(kinds)]
                c = _c(("ptr", "general")[i % 2], 1, H, W, C, N, kt, ks, hist=i % 3 != 0)
                if _flops(c) <= FLOP_CAP:
                    break
            imp.append(c)
            i += 1
    i = 0
    for H in (1, 7, 8, 9, 17):
        for W in (1, 31, 32, 33, 65):
            t_out, off = (1, 2, 3, 4, 5, 9)[i % 6], (0, 2)[i % 2]
            N = (96, 96, 8, 96, 16)[i % 5]
            c = _c("c96", off + t_out, H, W, 96, N, 3, 3, t_off=off, t_out=t_out, hist=i % 4 != 3)
            if _flops(c) > FLOP_CAP:
                c = dict(c, N=8)
            c96.append(c)
            i += 1
    i = 0
    for Hs in (4, 8, 12):
        for Ws in (16, 32, 48):
            t_out, off = 1 + i % 4, i % 2
            while _flops(_c("up", off + t_out, Hs, Ws, 192, 96, 1, 3, mode=1, t_off=off, t_out=t_out)) > FLOP_CAP:
                t_out -= 1
            up.append(_c("up", off + t_out, Hs, Ws, 192, 96, 1, 3, mode=1, t_off=off, t_out=t_out))
            i += 1
    i = 0
    combos = [(384, 3), (192, 1), (384, 1), (192, 3)]
    for T, H, W in ((1, 1, 1), (1, 14, 14), (1, 14, 15), (2, 9, 13), (3, 6, 30)):
        for N in (96, 192, 200, 384):
            for shift in range(4):
                C, kt = combos[(i + shift) % 4]
                c = _c("padded", T, H, W, C, N, kt, 3, hist=kt == 3 and i % 3 != 2)
                if _flops(c) <= FLOP_CAP:
                    break
            pad.append(c)
            i += 1
    return imp, c96, up, pad


def _merge(hand, grid):
    seen = {case_id(c) for c in hand}
    return hand + [c for c in grid if case_id(c) not in seen and not seen.add(case_id(c))]


def case_id(c):
    extra = "".join(f"-{k}{c[k]}" for k in ("mode", "t_stride", "t_off", "t_out", "kpad", "fill") if k in c) + ("" if c.get("hist", True) else "-nohist")
    return f"{c['route']}-T{c['T']}H{c['H']}W{c['W']}C{c['C']}N{c['N']}k{c['kt']}{c['ks']}{extra}"


_G = _grids()
IMPLICIT_CASES, C96_CASES, UP_CASES, PADDED_CASES = (_merge(h, g) for h, g in zip((IMPLICIT_CASES, C96_CASES, UP_CASES, PADDED_CASES), _G))
CONV_CASES = IMPLICIT_CASES + C96_CASES + UP_CASES + PADDED_CASES
assert all(_flops(c) <= FLOP_CAP for c in CONV_CASES)
CLASSES = ("selector", "integers", "gauss")


def case_inputs(c, cls):
    kw = {k: v for k, v in c.items() if k not in ("route", "fill")}
    return conv_inputs(cls, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# RMS_norm (+ SiLU)
def rmsnorm_silu_chain(x, gamma, silu):
    xd = x.double()
    C = x.shape[-1]
    n = rb(torch.sqrt(xd.pow(2).sum(-1, keepdim=True))).clamp_min(1e-12)
    y1 = rb(xd / n)
    y2 = rb((y1 * float(torch.tensor(float(C), dtype=torch.float32).sqrt())).float().double())     # fp32 product, then bf16
    y3 = rb(y2 * gamma.double())
    return rb(act_ref(y3, "silu")) if silu else y3


def rmsnorm_silu_f32(x, gamma, silu, fault=None):
    xf = x.float()
    C = x.shape[-1]
    s = (xf * xf).sum(-1, keepdim=True)
    n = torch.sqrt(s)
    if fault != "norm_not_rounded":
        n = rb(n)
    n = n.clamp_min(1e-12)
    sc = torch.tensor(float(C), dtype=torch.float32).sqrt()
    y2 = rb(xf / n * sc) if fault == "scale_before_rounding" else rb(rb(xf / n) * sc)
    y3 = rb(y2 * gamma.float())
    if silu:
        y3 = y3 / (1.0 + torch.exp(-y3))
    return y3.to(BF)


def _boundary_distance(v):
    """Relative distance of positive fp64 values from the nearest bf16 rounding boundary (the midpoint of two neighbours)."""
    e = torch.floor(torch.log2(v.clamp_min(1e-300)))
    frac = v / torch.exp2(e - 7)                                      # in units of the bf16 spacing: 128 .. 256
    return ((frac - torch.floor(frac)) - 0.5).abs() / frac


RMS_SPECIAL = ("zero", "constant", "spike", "up30", "down30")


def rms_inputs(rows, C, seed=0, sigma=3.0):
    """x [rows, C] bf16 Gaussian x `sigma` and gamma [C]; with 37 rows or more, rows 5 .. 9 are RMS_SPECIAL: all zero (the clamp applies),
    constant, one element 2^15 times the rest, and rows scaled by 2^30 and 2^-30.  Every row is drawn again until fp64 sqrt(sum x^2)
    lies at least 2^-14 from a bf16 rounding boundary."""
    g = _gen(77 * C + rows + 1013 * seed)
    x = (torch.randn((rows, C), generator=g) * sigma).to(BF)
    special = rows >= 37

    def make(r, attempt):
        row = torch.randn(C, generator=g) * sigma
        kind = RMS_SPECIAL[r - 5] if special and 5 <= r < 10 else None
        if kind == "zero":
            row = torch.zeros(C)
        elif kind == "constant":
            row = torch.full((C,), 1.5 + 0.25 * attempt)
        elif kind == "spike":
            row[(3 * C) // 4] = 2.0 ** 15 * sigma
        elif kind == "up30":
            row = row * 2.0 ** 30
        elif kind == "down30":
            row = row * 2.0 ** -30
        return row.to(BF)
    if special:
        for r in range(5, 10):
            x[r] = make(r, 0)
    for attempt in range(1, 200):
        nrm = torch.sqrt(x.double().pow(2).sum(-1))
        bad = torch.nonzero((nrm > 0) & (_boundary_distance(nrm) < 2.0 ** -14)).flatten().tolist()
        if not bad:
            gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(BF)
            return x, gamma
        for r in bad:
            x[r] = make(r, attempt)
    raise RuntimeError(f"rms_inputs({rows}, {C}): no draw keeps every row's norm clear of the rounding boundaries")


# C: every lanes-per-row instantiation (<= 64: 8 lanes, <= 128: 16, <= 256: 32, else 64) with full and partly idle lane groups, and
# the three-chunk kernel's 96 / 192 / 384.  rows per wave = 64 / lanes
RMS_C = (8, 16, 24, 64, 72, 96, 128, 136, 192, 256, 264, 384, 512)
RMS_BIG = (65541, 264)        # 64 lanes per row, grid capped at 4096 workgroups x 4 rows, 4 row groups per trip: 65536 rows a trip


def rms_lanes(C):
    return 8 if C <= 64 else (16 if C <= 128 else (32 if C <= 256 else 64))


def rms_rows(C):
    rpw = 64 // rms_lanes(C)
    return sorted({1, max(rpw - 1, 1), rpw, rpw + 1, 37})


# ---------------------------------------------------------------------------------------------------------------------
# softmax rows
def softmax_rows_chain(x, scale, bias, nvalid, ldo):
    """x [rows, ncols] bf16 (columns >= nvalid are never read), scale a Python float taken as fp32 -> (p, bound) fp64 [rows, ldo]."""
    rows, ncols = x.shape
    sc = float(torch.tensor(scale, dtype=torch.float32))
    a = x[:, :nvalid].double() * sc
    exact_arg = bias is not None
    if bias is not None:
        a = rb(a + bias[:, :nvalid].double())
    mx = a.amax(-1, keepdim=True)
    e = torch.exp(a - mx)
    p = e / e.sum(-1, keepdim=True)
    u = 2.0 ** -24
    dc = u * ((0.0 if exact_arg else 1.0) * a.abs() + mx.abs() + (a - mx).abs())
    r = 1.01 * (dc + dc.amax(-1, keepdim=True)) + (10 + nvalid) * u
    out, bound = torch.zeros((rows, ldo), dtype=torch.float64), torch.zeros((rows, ldo), dtype=torch.float64)
    out[:, :nvalid] = p
    bound[:, :nvalid] = 2.0 ** -8 * p * (1 + r) + r * p + 2.0 ** -126
    return out, bound


def softmax_rows_f32(x, scale, bias, nvalid, ldo, fault=None):
    rows, ncols = x.shape
    sc = torch.tensor(scale, dtype=torch.float32)
    v = x.float() * sc
    if bias is not None:
        v = v + bias.float() if fault == "bias_without_rounding" else rb(v + bias.float())
    mx = (v if fault == "max_over_ncols" else v[:, :nvalid]).amax(-1, keepdim=True)
    e = torch.exp(v[:, :nvalid] - mx)
    out = torch.zeros((rows, ldo), dtype=torch.float32)
    out[:, :nvalid] = e * (1.0 / e.sum(-1, keepdim=True))
    return out.to(BF)


def softmax_judge(got, p, bound):
    """-> (elements outside the bound, worst |got - p| / bound, pad exactly zero)."""
    err = (got.double() - p).abs()
    live = bound > 0
    bad = ~(err <= bound)
    ratio = torch.where(live, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return int(bad.sum()), float(torch.nan_to_num(ratio, nan=math.inf).max()), bool((bits(got)[~live] == 0).all())


SOFTMAX_NCOLS = (1, 24, 255, 256, 257, 1560)
SOFTMAX_STD = (1.0, 8.0, 50.0)
MASKED = 1e30        # what the columns from nvalid to ncols hold: the reference masks them, the kernel must not read them


def softmax_cases():
    """(ncols, nvalid, with bias, score std): every ncols with nvalid 1 / ncols - 1 / ncols, with and without a bias, the stds in turn."""
    out = []
    for i, nc in enumerate(SOFTMAX_NCOLS):
        for k, nv in enumerate(sorted({1, max(nc - 1, 1), nc})):
            for b in (False, True):
                out.append((nc, nv, b, SOFTMAX_STD[(i + k + b) % 3]))
    return out


def softmax_inputs(ncols, nvalid, with_bias, std, rows=5):
    """x [rows, ncols] bf16 scores of std `std` (row 3: all equal; columns >= nvalid: MASKED), the scale (1 with a bias, as umT5 calls it:
    x scale + bias is then a sum of two bf16 values, exact in fp32, and is asserted to round alike in fp32 and fp64; 0.3 without — not a
    power of two, so the fp32 product rounds) and the bias (a fifth of the scores' std) or None."""
    g = _gen(13 * ncols + nvalid + 7 * with_bias + int(std))
    x = (torch.randn((rows, ncols), generator=g) * std)
    x[3] = 0.75 * std
    x[:, nvalid:] = MASKED
    x = x.to(BF)
    if not with_bias:
        return x, 0.3 * (1.0 if std < 50 else 3.0), None
    # both on a grid (x: 2^-8, bias: 2^-4) so that their sum spans at most 2^9 .. 2^-8: 17 bits, exact in fp32
    x = torch.where(x.float().abs() < MASKED / 2, (x.float() * 256).round() / 256, x.float()).to(BF)
    bias = ((torch.randn((rows, ncols), generator=g) * std / 5) * 16).round().div(16).to(BF)
    a32, a64 = x.float() + bias.float(), x.double() + bias.double()
    assert torch.equal(a32[:, :nvalid].double(), a64[:, :nvalid]), "x + bias must be exact in fp32"
    return x, 1.0, bias


# ---------------------------------------------------------------------------------------------------------------------
# the latent scale steps
def prep_latent_ref(z, mean, inv_std, cpad):
    """z [C, T, H, W] bf16 -> channels-last [T, H, W, cpad]: bf16(bf16(z / inv_std) + mean), channels >= C zero."""
    C = z.shape[0]
    v = rb(z.float() / inv_std.float()[:, None, None, None]) + mean.float()[:, None, None, None]
    out = torch.zeros(tuple(z.shape[1:]) + (cpad,), dtype=BF)
    out[..., :C] = v.to(BF).permute(1, 2, 3, 0)
    return out


def finish_latent_ref(x, mean, inv_std, C):
    """x [rows, >= C] bf16 -> [rows, C]: bf16(bf16(x - mean) inv_std)."""
    return (rb(x[:, :C].float() - mean.float()) * inv_std.float()).to(BF)
