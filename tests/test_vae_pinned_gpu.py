"""The VAE's hand-written kernels pinned element by element against references that are not this project's own gather
(tests/vae_refs.py): the patch gather gf_vae_im2col against `unfold` of the plainly padded tensor, and every convolution kernel —
both gathers of gf_conv3d_bf16 (gemm_ph_kernel<CONV = 1, 2>), the direct 96-channel and the direct upsample kernel
(gf_conv_direct.hip), gf_conv3d_padded_bf16 (gf_conv_a4.hip) — against a plain fp64 F.conv3d written from the reference's
CausalConv3d / Resample, at the edges of each kernel's own tiling, through the raw C ABI, on three data classes:

  selector   one +-2^k per weight row, cycling through all taps: every output is one shifted input element; torch.equal with the chain;
  integers   small integers, exact accumulators in every order: torch.equal with the chain, both epilogues;
  gauss      Gaussian operands through gemm_refs' two bars: (a) differing bf16 bits on <= 2^-10 of the output and per row / column at
             most the binomial cap, (b) every element within 2^-7 m + K 2^-23 S.

Every convolution runs inside NaN-filled parents (the memory in front of the history, every frame the window does not read, the gap
of `resid`), with sentinel guards in the gap of `out` and behind its last row.  The row kernels of gf_vae.hip: gf_vae_rmsnorm_silu
(torch.equal with its chain when silu = False; the SiLU within one bf16 step), gf_softmax_rows (a derived per-element bound),
gf_vae_prep_latent / gf_vae_finish_latent (bit for bit against their fp32 formulas).  tests/test_vae_refs_cpu.py shows on the CPU
that a right computation is inside every bar on these very inputs and that thirteen injected faults are not.  Every comparison prints
what it measured (`pytest -s`); the last test prints the figures per kernel.

Measured on an MI355X (gauss class; share = differing bf16 bits against the chain, cap 9.77e-4; ratio = the worst element's share of the
allowance of bar (b); worst row / column count of its binomial cap; profiles/r17/README.md has every line):
  general gather (CONV = 1)        54 comparisons   share 1.44e-4   ratio 0.901   row 1 of 5   column 2 of 9
  pointer-per-row gather (CONV = 2) 54              share 2.64e-4   ratio 0.637   row 2 of 8   column 2 of 7
  direct 96-channel                66               share 2.88e-4   ratio 0.598   row 2 of 5   column 3 of 15
  direct upsample                  14               share 1.63e-4   ratio 0.808   row 2 of 5   column 3 of 15
  padded layout                    52               share 3.72e-4   ratio 0.761   row 2 of 5   column 2 of 7
  selector and integers: equal to the chain everywhere, on every kernel and fall-back; gf_vae_im2col equal to unfold in 228 gathers.
  gf_vae_rmsnorm_silu: equal to the chain in 76 comparisons (65541 x 264 among them), SiLU 0 bf16 steps from bf16(fp64);
  gf_softmax_rows: worst element 0.988 of its bound (the bound is the final rounding's 2^-8 p to within 1 %);
  gf_vae_prep_latent / gf_vae_finish_latent: 0 values differ from the fp32 formulas — the device division is correctly rounded.
Found: no kernel fault.

Departures from the issue, each because the C ABI refuses the shape (the refusals are tested here by message):
  * gf_vae_im2col / gf_conv3d_bf16 refuse mode 2 on an odd H or W, so the odd 5 x 7 image is a refusal case, not a gather case;
  * gf_conv3d_bf16 takes N in multiples of 8, so the RGB-head instantiation is reached at N = 8 and 16 (not 4, 12) and the fall-back
    width is N = 24 (not 20); N = 4, 12 and 20 are refusal cases.
"""
import pytest
import torch

import forward_refs as FR
import gemm_refs as R
import vae_refs as V

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENT = 0x5A5A                       # a finite bf16 bit pattern (1.5e16) no output here comes near
FIG = {}
_CACHE = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from goal_force_amd import ops as _ops
    assert (_ops.lib_option("conv_direct"), _ops.lib_option("conv_gather"), _ops.lib_option("conv_nb"), _ops.lib_option("vae_rms3")) == (1, 0, 0, 1), "the shipped dispatch"
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    return ops._lib.load()


@pytest.fixture(autouse=True)
def _no_grad(request):
    """No autograd; the cached cases (inputs, fp64 references) live only while the parametrised cases of ONE test function run."""
    name = request.node.originalname
    if _CACHE.get("_owner") != name:
        _CACHE.clear()
        _CACHE["_owner"] = name
    with torch.no_grad():
        yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                   # a device fault: nothing more is started on the GPU
        pytest.exit(f"the GPU reported a fault after {request.node.nodeid}: {e}", returncode=3)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16)


def _sentinel(shape):
    t = torch.empty(shape, dtype=BF, device="cuda")
    t.view(torch.int16).fill_(SENT)
    return t


def _intact(t):
    return bool((_bits(t) == SENT).all())


def _nan(shape):
    return torch.full(shape, float("nan"), dtype=BF, device="cuda")


def _err(lib):
    return lib.gf_last_error().decode("utf-8", "replace")


def _case(c, cls):
    key = (V.case_id(c), cls)
    if key not in _CACHE:
        _CACHE[key] = V.case_inputs(c, cls)
    return _CACHE[key]


def _note(form, j):
    f = FIG.setdefault(form, dict(cases=0, share=0.0, worst=0.0, row=(0, 0), col=(0, 0)))
    f["cases"] += 1
    f["share"], f["worst"] = max(f["share"], j["share"]), max(f["worst"], j["worst"])
    if j["row_worst"] * max(f["row"][1], 1) >= f["row"][0] * j["row_cap"]:
        f["row"] = (j["row_worst"], j["row_cap"])
    if j["col_worst"] * max(f["col"][1], 1) >= f["col"][0] * j["col_cap"]:
        f["col"] = (j["col_worst"], j["col_cap"])


def _judge(d, epi, got, form, what):
    """One output against its chain by the class's bar."""
    ref = V.conv_ref(d, epi)
    what = f"{form} {d['cls']} {d['what']} {R.EPI_NAMES[epi]} {what}"
    if d["cls"] == "gauss":
        _note(form, R.assert_pinned(got, ref, V.conv_k(d), what))
        return
    diff = R.bits(got) != R.bits(ref.out)
    if bool(diff.any()):
        idx = torch.nonzero(diff)
        row, n = idx[0].tolist()
        where = V.selector_explain(d, row, n) if d["cls"] == "selector" else f"first (row, column) {idx[:6].tolist()}"
        raise AssertionError(f"{what}: {idx.shape[0]} of {diff.numel()} elements differ from the chain; {where}: got {float(got[row, n])}, "
                             f"chain {float(ref.out[row, n])}")


# ---------------------------------------------------------------------------------------------------------------------
# launching a convolution inside NaN-filled parents and guarded outputs, through the raw C ABI
def _activation(d, route):
    """-> (src, cache): device pointers' tensors.  One parent [1 + 2 + T + 1, H, W, C] of NaN: frame 0 stays NaN (the memory in front of
    the history), frames 1, 2 hold the history when it lies in front of src (NaN otherwise), then x — its frames outside every window
    NaN — and a NaN frame behind.  A separate cache sits in a NaN parent of its own."""
    x, hist, kt = d["x"], d["hist"], d["kt"]
    T, H, W, C = x.shape
    parent = _nan((T + 4, H, W, C))
    xd = x.cuda()
    read = set(V.frames_read(kt, d["t_stride"], d["t_off"], d["t_out"]))
    for f in range(T):
        if f in read:
            parent[3 + f] = xd[f]
    cache = None
    if kt == 3:
        h = torch.zeros((2, H, W, C), dtype=BF) if hist is None else hist
        if route == "general":
            cpar = _nan((4, H, W, C))
            cpar[1:3] = h.cuda()
            cache = cpar[1:3]
        else:
            parent[1:3] = h.cuda()
        for f in (-2, -1):                                             # a history frame no window reads (t_off > 0)
            if f not in read:
                (cache if route == "general" else parent[1:3])[2 + f] = float("nan")
    return parent[3:3 + T], cache


def _opts(route, d):
    if route == "general":
        return dict(conv_direct=0, conv_gather=1)
    if route == "ptr":
        return dict(conv_direct=0, conv_gather=0)
    return dict(conv_direct=1, conv_gather=0)


def _conv(ops, lib, d, route, epi, bias=True, gap=8):
    """gf_conv3d_bf16 on a case dict -> (out [rows, N] on the CPU, the whole guarded buffer)."""
    T, H, W, C, N = d["shape"]
    Ho, Wo = V.out_hw(H, W, d["mode"])
    rows = d["t_out"] * Ho * Wo
    src, cache = _activation(d, route)
    w = d["w"].cuda()
    b = d["bias"].cuda() if bias else None
    ldc = N + gap
    out = _sentinel((rows + 1, ldc))
    resid = None
    if epi == R.EPI_RESID:
        resid = _nan((rows, ldc))
        resid[:, :N] = d["resid"].cuda()
    with ops.options(**_opts(route, d)):
        rc = lib.gf_conv3d_bf16(src.data_ptr(), None if cache is None else cache.data_ptr(), w.data_ptr(), w.stride(0),
                                None if b is None else b.data_ptr(), out.data_ptr(), ldc, T, d["t_out"], H, W, C, d["kt"], d["ks"], d["mode"],
                                d["t_stride"], d["t_off"], N, w.shape[1], ops.EPI_BIAS if resid is None else ops.EPI_BIAS_RESID,
                                None if resid is None else resid.data_ptr(), ldc if resid is not None else 0, _st())
    assert rc == 0, f"gf_conv3d_bf16 {d['what']}: status {rc}: {_err(lib)}"
    torch.cuda.synchronize()
    assert _intact(out[rows:]) and _intact(out[:, N:]), f"{route} {d['what']}: wrote outside [rows, N] of out (ldc = {ldc})"
    return out[:rows, :N].cpu(), out


def _padded_buffer(ops, d, fill):
    """The zero-bordered input of gf_conv3d_padded_bf16 inside a NaN parent, its interior written by a copy, by
    gf_vae_rmsnorm_silu_padded or by gf_vae_upsample2x_padded; -> (buf, the case dict whose x is what the interior now holds)."""
    T, H, W, C, N = d["shape"]
    kt = d["kt"]
    parent = _nan((kt - 1 + T + 2, H + 2, W + 2, C))
    buf = parent[1:kt + T]
    buf.zero_()
    if kt == 3 and d["hist"] is not None:
        buf[:2, 1:H + 1, 1:W + 1] = d["hist"].cuda()
    interior = buf[kt - 1:, 1:H + 1, 1:W + 1]
    if fill == "rms":
        g = torch.Generator().manual_seed(5)
        pre = (torch.randn((T, H, W, C), generator=g) * 2.5).to(BF).cuda()
        gam = (1 + 0.1 * torch.randn(C, generator=g)).to(BF).cuda()
        view = ops.vae_rmsnorm_silu_padded(pre, gam, buf, silu=True)
        assert view.data_ptr() == interior.data_ptr() and torch.equal(view, ops.vae_rmsnorm_silu(pre, gam, silu=True))
    elif fill == "up":
        g = torch.Generator().manual_seed(6)
        half = (torch.randn((T, H // 2, W // 2, C), generator=g) * 0.7).to(BF).cuda()
        view = ops.vae_upsample2x_padded(half, buf)
        assert view.data_ptr() == interior.data_ptr() and torch.equal(view, half.repeat_interleave(2, 1).repeat_interleave(2, 2))
    else:
        interior.copy_(d["x"].cuda())
    if fill != "copy":
        d = {k: v for k, v in d.items() if not k.startswith("_")}
        d["x"] = interior.cpu().contiguous()
    return parent, buf, d


def _border_is_zero(parent, buf, H, W):
    return (float(buf[:, 0].float().abs().sum()) == 0 and float(buf[:, H + 1].float().abs().sum()) == 0 and float(buf[:, :, 0].float().abs().sum()) == 0
            and float(buf[:, :, W + 1].float().abs().sum()) == 0 and bool(torch.isnan(parent[0].float()).all()) and bool(torch.isnan(parent[-1].float()).all()))


def _conv_padded(ops, lib, d, buf, epi, bias=True, gap=8):
    T, H, W, C, N = d["shape"]
    rows = T * H * W
    w = d["w"].cuda()
    b = d["bias"].cuda() if bias else None
    ldo = N + gap
    out = _sentinel((rows + 1, ldo))
    resid = None
    if epi == R.EPI_RESID:
        resid = _nan((rows, ldo + 8))
        resid[:, :N] = d["resid"].cuda()
    rc = lib.gf_conv3d_padded_bf16(buf.data_ptr(), w.data_ptr(), w.stride(0), None if b is None else b.data_ptr(), out.data_ptr(), ldo, T, H, W, C, N,
                                   d["kt"], ops.EPI_BIAS if resid is None else ops.EPI_BIAS_RESID, None if resid is None else resid.data_ptr(),
                                   ldo + 8 if resid is not None else 0, _st())
    assert rc == 0, f"gf_conv3d_padded_bf16 {d['what']}: status {rc}: {_err(lib)}"
    torch.cuda.synchronize()
    assert _intact(out[rows:]) and _intact(out[:, N:]), f"padded {d['what']}: wrote outside [rows, N] of out (ldo = {ldo})"
    return out[:rows, :N].cpu()


# ---------------------------------------------------------------------------------------------------------------------
# the patch gather
IM2COL_HW = {0: [(1, 1), (1, 7), (7, 1), (5, 6), (9, 11)], 1: [(1, 1), (1, 7), (7, 1), (5, 6), (9, 11)], 2: [(2, 2), (4, 6), (6, 4), (10, 12)]}
WINDOWS = [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]          # (t_stride, t_off)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_im2col_equals_unfold_of_the_plainly_padded_tensor(ops, mode):
    """gf_vae_im2col, every mode x (kt, ks) x (t_stride, t_off) x C 8 / 24 / 96 x image sizes from one pixel up, kpad = k and > k: equal
    to `unfold` of the padded tensor; the pad columns exactly zero; source frames outside the window, and the memory around the
    cache, are NaN."""
    n = 0
    for kt, ks in ((3, 3), (1, 3), (3, 1), (1, 1)):
        if mode != 0 and ks != 3:
            continue
        for hi, (H, W) in enumerate(IM2COL_HW[mode]):
            for wi, (ts, off) in enumerate(WINDOWS):
                C = (8, 24, 96)[(hi + wi + kt) % 3]
                t_out = 1 + (hi + wi) % 2
                T = off + (t_out - 1) * ts + 1 + (wi % 2)                    # sometimes a frame behind the window
                k = kt * ks * ks * C
                kpad = k + (0, 8, 56)[(hi + wi) % 3]
                d = V.conv_inputs("selector", T, H, W, C, 8, kt, ks, mode, ts, off, t_out, seed=n)
                src, cache = _activation(d, "general")
                got = ops.vae_im2col(src, cache, kt, ks, kpad, upsample2x=mode == 1, downsample2=mode == 2, t_stride=ts, t_off=off, t_out=t_out).cpu()
                want = V.patches(d["x"], d["hist"], kt, ks, mode, ts, off, t_out)
                what = f"mode {mode} kt {kt} ks {ks} H {H} W {W} C {C} t_stride {ts} t_off {off} t_out {t_out} kpad {kpad}"
                assert got.shape == (want.shape[0], kpad), what
                assert torch.equal(_bits(got[:, :k]), _bits(want)), f"{what}: {int((_bits(got[:, :k]) != _bits(want)).sum())} of {want.numel()} differ"
                assert bool((_bits(got[:, k:]) == 0).all()), f"{what}: the pad columns are not zero"
                n += 1
    print(f"PIN gf_vae_im2col mode {mode}: {n} gathers equal to unfold")


# ---------------------------------------------------------------------------------------------------------------------
# the convolution kernels
def _ids(cases):
    return [V.case_id(c) for c in cases]


@pytest.mark.parametrize("cls", V.CLASSES)
@pytest.mark.parametrize("c", V.IMPLICIT_CASES, ids=_ids(V.IMPLICIT_CASES))
def test_implicit_gemm_both_gathers(ops, lib, c, cls):
    """gf_conv3d_bf16 with conv_direct = 0: the general gather (a separate cache, modes 1 and 2, or conv_gather = 1) and the
    pointer-per-row gather (history in front, or kt = 1 with mode 0), both epilogues, ldc = ldr = N + 8."""
    d = _case(c, cls)
    for epi in V.EPIS:
        got, _ = _conv(ops, lib, d, c["route"], epi)
        _judge(d, epi, got, "implicit " + c["route"], "")


@pytest.mark.parametrize("cls", V.CLASSES)
@pytest.mark.parametrize("c", V.C96_CASES, ids=_ids(V.C96_CASES))
def test_direct_96_channel_kernel(ops, lib, c, cls):
    """The direct kernel (contiguous rows: ldc = ldr = N) at its patch and segment edges, and its fall-backs (ldc = N + 8; N = 24)."""
    d = _case(c, cls)
    for epi in V.EPIS:
        got, _ = _conv(ops, lib, d, "c96", epi, gap=0)
        _judge(d, epi, got, "direct c96" if c["N"] != 24 else "c96 fall-back N 24", "")
    if c["N"] == 96 and c["H"] == 8:
        for epi in V.EPIS:
            got, _ = _conv(ops, lib, d, "c96", epi, gap=8)
            _judge(d, epi, got, "c96 fall-back ldc", "ldc N + 8")


@pytest.mark.parametrize("cls", V.CLASSES)
@pytest.mark.parametrize("c", V.UP_CASES, ids=_ids(V.UP_CASES))
def test_direct_upsample_kernel(ops, lib, c, cls):
    """The direct 192 -> 96 upsample kernel (bias epilogue, ldc = N) and what falls back beside it (the residual epilogue, Hs % 4,
    Ws % 16): all equal the chain."""
    d = _case(c, cls)
    direct = c["H"] % 4 == 0 and c["W"] % 16 == 0
    for epi in V.EPIS:
        got, _ = _conv(ops, lib, d, "up", epi, gap=0)
        _judge(d, epi, got, "direct up" if direct and epi == R.EPI_BIAS else "up fall-back", "")


@pytest.mark.parametrize("cls", V.CLASSES)
@pytest.mark.parametrize("c", V.PADDED_CASES, ids=_ids(V.PADDED_CASES))
def test_padded_layout_kernel(ops, lib, c, cls):
    """gf_conv3d_padded_bf16 around its 256-row tile, ldo = N + 8 and ldr = N + 16, a non-zero history; the gauss class's interior is
    written by the case's producer (copy, gf_vae_rmsnorm_silu_padded, gf_vae_upsample2x_padded) and the border is exactly zero
    afterwards."""
    d0 = _case(c, cls)
    T, H, W, C, N = d0["shape"]
    fill = c.get("fill", "copy") if cls == "gauss" else "copy"
    key = ("padded", V.case_id(c), cls)
    if key not in _CACHE:
        _CACHE[key] = _padded_buffer(ops, d0, fill)
    parent, buf, d = _CACHE[key]
    for epi in V.EPIS:
        got = _conv_padded(ops, lib, d, buf, epi)
        _judge(d, epi, got, "padded", f"fill {fill}")
    assert _border_is_zero(parent, buf, H, W), "the zero border or the NaN frames around the buffer were written"


ONE_PER_KERNEL = [V.IMPLICIT_CASES[9], V.IMPLICIT_CASES[3], V.C96_CASES[2], V.UP_CASES[0], V.PADDED_CASES[5]]


@pytest.mark.parametrize("c", ONE_PER_KERNEL, ids=_ids(ONE_PER_KERNEL))
def test_null_bias_is_a_zero_bias(ops, lib, c):
    d = dict(V.case_inputs(c, "gauss"))
    zero = dict(d, bias=torch.zeros_like(d["bias"]))
    for epi in V.EPIS:
        if c["route"] == "padded":
            _, buf, _ = _padded_buffer(ops, d, "copy")
            a, b = _conv_padded(ops, lib, d, buf, epi, bias=False), _conv_padded(ops, lib, zero, buf, epi)
        else:
            gap = 0 if c["route"] in ("c96", "up") else 8
            a, b = _conv(ops, lib, d, c["route"], epi, bias=False, gap=gap)[0], _conv(ops, lib, zero, c["route"], epi, gap=gap)[0]
        assert torch.equal(_bits(a), _bits(b)), f"{V.case_id(c)} {R.EPI_NAMES[epi]}: bias = NULL differs from a zero bias"
        _judge(zero, epi, b, "null bias", V.case_id(c))


# ---------------------------------------------------------------------------------------------------------------------
# refusals
def _refused(lib, rc, fn, text, out, what):
    assert rc != 0, f"{what}: accepted"
    assert _err(lib).startswith(fn + ":") and text in _err(lib), f"{what}: message {_err(lib)!r} is not {fn}'s {text!r}"
    torch.cuda.synchronize()
    assert _intact(out), f"{what}: the output was touched"


def test_refusals_leave_the_output_untouched(ops, lib):
    x = torch.zeros((4, 4, 4, 16), dtype=BF, device="cuda")
    cache = torch.zeros((2, 4, 4, 16), dtype=BF, device="cuda")
    w = torch.zeros((8, 448), dtype=BF, device="cuda")
    b = torch.zeros((8,), dtype=BF, device="cuda")
    out = _sentinel((256, 448))
    p, st = lambda t: t.data_ptr(), _st()       # noqa: E731

    def im2col(src=p(x), ca=p(cache), o=p(out), T_out=2, H=4, W=4, C=16, kt=3, ks=3, mode=0, ts=1, off=0, kpad=448):
        return lib.gf_vae_im2col(src, ca, o, T_out, H, W, C, kt, ks, mode, ts, off, kpad, st)
    for kw, text in ((dict(src=None), "bad arguments"), (dict(o=None), "bad arguments"), (dict(T_out=0), "bad arguments"), (dict(H=0), "bad arguments"),
                     (dict(C=12, kpad=328), "must be a multiple of 8"), (dict(kpad=424), "must be a multiple of 8"), (dict(kpad=444), "must be a multiple of 8"),
                     (dict(kt=2), "kernel must be 1 or 3"), (dict(ks=2), "kernel must be 1 or 3"), (dict(mode=3), "bad mode"), (dict(ts=0), "bad mode"),
                     (dict(off=-1), "bad mode"), (dict(mode=2, H=5, W=7), "even H, W"), (dict(mode=2, kt=1, ks=1, kpad=16), "even H, W and ks=3"),
                     (dict(ca=None), "needs the 2-frame cache"), (dict(src=p(x) + 2), "16-byte alignment"), (dict(o=p(out) + 2), "16-byte alignment"),
                     (dict(ca=p(cache) + 2), "16-byte alignment")):
        _refused(lib, im2col(**kw), "gf_vae_im2col", text, out, f"gf_vae_im2col {kw}")
    assert im2col() == 0                                                       # and the call they were all made from is accepted
    torch.cuda.synchronize()
    out = _sentinel((256, 448))
    resid = torch.zeros((256, 8), dtype=BF, device="cuda")

    def conv(src=p(x), ca=p(cache), wm=p(w), ldw=448, bias=p(b), o=p(out), ldc=8, T_in=4, T_out=2, H=4, W=4, C=16, kt=3, ks=3, mode=0, ts=1, off=0,
             N=8, K=448, epi=ops.EPI_BIAS, r=None, ldr=0):
        return lib.gf_conv3d_bf16(src, ca, wm, ldw, bias, o, ldc, T_in, T_out, H, W, C, kt, ks, mode, ts, off, N, K, epi, r, ldr, st)
    for kw, text in ((dict(src=None), "null src/W/out"), (dict(wm=None), "null src/W/out"), (dict(o=None), "null src/W/out"),
                     (dict(T_in=0), "bad frame size"), (dict(T_out=-1), "bad frame size"), (dict(H=32768), "bad frame size"), (dict(W=0), "bad frame size"),
                     (dict(C=12), "must be a multiple of 8 and <= 512"), (dict(C=520), "must be a multiple of 8 and <= 512"),
                     (dict(kt=2), "kt/ks must be 1 or 3"), (dict(ks=2), "kt/ks must be 1 or 3"), (dict(mode=3), "bad mode"),
                     (dict(mode=1, kt=1, ks=1, K=64), "bad mode"), (dict(mode=2, kt=1, H=5, W=7, K=192), "stride-2 mode needs even H, W"),
                     (dict(ts=0), "reach past the input"), (dict(off=-1), "reach past the input"), (dict(off=3), "reach past the input"),
                     (dict(T_out=3, ts=2), "reach past the input"), (dict(K=440), "must be a multiple of 64 covering"),
                     (dict(K=384), "must be a multiple of 64 covering"), (dict(ldw=384), "must be a multiple of 64 covering"),
                     (dict(ldw=452), "must be a multiple of 64 covering"), (dict(K=65536, ldw=65536), "must be a multiple of 64 covering"),
                     (dict(N=0), "N / ldc must be multiples of 8"), (dict(N=4, ldc=4), "N / ldc must be multiples of 8"),
                     (dict(N=12, ldc=16), "N / ldc must be multiples of 8"), (dict(N=20, ldc=24), "N / ldc must be multiples of 8"),
                     (dict(ldc=4), "N / ldc must be multiples of 8"), (dict(ldc=12), "N / ldc must be multiples of 8"),
                     (dict(src=p(x) + 2), "16-byte alignment"), (dict(wm=p(w) + 2), "16-byte alignment"), (dict(o=p(out) + 2), "16-byte alignment"),
                     (dict(ca=p(cache) + 2), "16-byte alignment"), (dict(bias=p(b) + 2), "16-byte alignment"),
                     (dict(epi=ops.EPI_BIAS_SILU), "epilogue must be BIAS or BIAS_RESID"), (dict(epi=ops.EPI_BIAS_GATE_RESID), "epilogue must be BIAS or BIAS_RESID"),
                     (dict(epi=ops.EPI_BIAS_RESID), "residual epilogue needs"), (dict(epi=ops.EPI_BIAS_RESID, r=p(resid), ldr=4), "residual epilogue needs"),
                     (dict(epi=ops.EPI_BIAS_RESID, r=p(resid), ldr=12), "residual epilogue needs"),
                     (dict(epi=ops.EPI_BIAS_RESID, r=p(resid) + 2, ldr=8), "residual epilogue needs"),
                     (dict(H=32767, W=32767, T_in=2, T_out=2, kt=1, ks=1, K=64), "too many output pixels")):
        _refused(lib, conv(**kw), "gf_conv3d_bf16", text, out, f"gf_conv3d_bf16 {kw}")
    assert conv() == 0 and conv(T_out=0) == 0                                  # accepted; no output frames: a no-op
    torch.cuda.synchronize()
    assert _intact(out[32:]) and not _intact(out[:32, :8])
    # the module-side wrapper's own refusals
    with pytest.raises(ops.GoalForceError, match="history_in_front"):
        ops.vae_conv3d(x.clone(), None, w, None, 3, 3, history_in_front=True)
    with pytest.raises(ops.GoalForceError, match="temporal window exceeds"):
        ops.vae_conv3d(x, None, w[:, :192], None, 1, 3, t_off=3, t_out=2)

    out = _sentinel((256, 200))
    xp = torch.zeros((4, 6, 6, 192), dtype=BF, device="cuda")
    wp = torch.zeros((96, 5184), dtype=BF, device="cuda")
    bp = torch.zeros((104,), dtype=BF, device="cuda")
    rp = torch.zeros((32, 96), dtype=BF, device="cuda")

    def padded(a=p(xp), wm=p(wp), ldw=5184, bias=p(bp), o=p(out), ldo=200, T=2, H=4, W=4, C=192, N=96, kt=3, epi=ops.EPI_BIAS, r=None, ldr=0):
        return lib.gf_conv3d_padded_bf16(a, wm, ldw, bias, o, ldo, T, H, W, C, N, kt, epi, r, ldr, st)
    for kw, text in ((dict(a=None), "bad arguments (kt = 1 or 3)"), (dict(wm=None), "bad arguments (kt = 1 or 3)"), (dict(o=None), "bad arguments (kt = 1 or 3)"),
                     (dict(T=0), "bad arguments (kt = 1 or 3)"), (dict(H=0), "bad arguments (kt = 1 or 3)"), (dict(kt=2), "bad arguments (kt = 1 or 3)"),
                     (dict(C=96), "outside the kernel's shapes"), (dict(C=200), "outside the kernel's shapes"), (dict(N=100), "outside the kernel's shapes"),
                     (dict(N=0), "outside the kernel's shapes"), (dict(epi=ops.EPI_BIAS_SILU), "epilogue must be BIAS or BIAS_RESID"),
                     (dict(epi=ops.EPI_BIAS_RESID), "epilogue must be BIAS or BIAS_RESID"), (dict(epi=ops.EPI_BIAS_RESID, r=p(rp), ldr=88), "epilogue must be BIAS or BIAS_RESID"),
                     (dict(epi=ops.EPI_BIAS_RESID, r=p(rp), ldr=100), "epilogue must be BIAS or BIAS_RESID"),
                     (dict(ldw=5176), "bad leading dimensions"), (dict(ldw=5188), "bad leading dimensions"), (dict(ldo=88), "bad leading dimensions"),
                     (dict(ldo=100), "bad leading dimensions"), (dict(a=p(xp) + 2), "16-byte alignment required (bias: 8)"),
                     (dict(wm=p(wp) + 2), "16-byte alignment required (bias: 8)"), (dict(o=p(out) + 2), "16-byte alignment required (bias: 8)"),
                     (dict(bias=p(bp) + 2), "16-byte alignment required (bias: 8)"), (dict(epi=ops.EPI_BIAS_RESID, r=p(rp) + 2, ldr=96), "16-byte alignment required (bias: 8)"),
                     (dict(T=1, H=4000, W=4000), "must each stay below 4 GiB")):
        _refused(lib, padded(**kw), "gf_conv3d_padded_bf16", text, out, f"gf_conv3d_padded_bf16 {kw}")
    assert padded() == 0 and padded(bias=p(bp) + 8) == 0                        # the bias needs 8-byte alignment only
    torch.cuda.synchronize()
    assert _intact(out[32:]) and _intact(out[:, 96:])

    x8 = torch.ones((3, 520), dtype=BF, device="cuda")
    o8 = _sentinel((3, 520))
    for C, text in ((520, "must be a multiple of 8 and <= 512"), (12, "must be a multiple of 8 and <= 512"), (0, "must be a multiple of 8 and <= 512")):
        _refused(lib, lib.gf_vae_rmsnorm_silu(p(x8), p(x8), p(o8), 3, C, 1, st), "gf_vae_rmsnorm_silu", text, o8, f"gf_vae_rmsnorm_silu C = {C}")
    _refused(lib, lib.gf_vae_rmsnorm_silu(p(x8) + 2, p(x8), p(o8), 3, 64, 1, st), "gf_vae_rmsnorm_silu", "alignment", o8, "gf_vae_rmsnorm_silu misaligned x")
    _refused(lib, lib.gf_vae_rmsnorm_silu(None, p(x8), p(o8), 3, 64, 1, st), "gf_vae_rmsnorm_silu", "bad arguments", o8, "gf_vae_rmsnorm_silu null x")


# ---------------------------------------------------------------------------------------------------------------------
# RMS_norm (+ SiLU)
def _rms_check(ops, x, gamma, what, run):
    """silu = False: torch.equal with the chain; silu = True: within one bf16 step of bf16(fp64 SiLU) of the kernel's own silu = False
    output, and the differing share against the chain <= 2^-10."""
    plain = run(False)
    want = V.rmsnorm_silu_chain(x, gamma, False)
    diff = R.bits(plain) != R.bits(want)
    assert not bool(diff.any()), f"{what}: {int(diff.sum())} of {diff.numel()} differ from the chain; first (row, column) {torch.nonzero(diff)[:4].tolist()}"
    act = run(True)
    FR.assert_act(act.reshape(-1), plain.reshape(-1), "silu", what + " silu")
    share = float((R.bits(act) != R.bits(V.rmsnorm_silu_chain(x, gamma, True))).double().mean())
    assert share <= R.SHARE_CAP, f"{what}: SiLU differs from the chain on {share:.2e} (cap 2^-10)"
    f = FIG.setdefault("rmsnorm_silu", dict(cases=0, share=0.0))
    f["cases"] += 1
    f["share"] = max(f["share"], share)


@pytest.mark.parametrize("C", V.RMS_C)
def test_rmsnorm_silu_every_width(ops, C):
    """gf_vae_rmsnorm_silu at every lanes-per-row instantiation, rows around a wave's row count and 37 (zero, constant, spike and
    2^+-30 rows among them); C = 96 / 192 / 384 on both kernels (vae_rms3 1 / 0); C = 192 / 384 into the padded layout as well."""
    for rows in V.rms_rows(C):
        x, gamma = V.rms_inputs(rows, C)
        xd, gd = x.cuda(), gamma.cuda()
        for rms3 in ((1, 0) if C in (96, 192, 384) else (1,)):
            with ops.options(vae_rms3=rms3):
                _rms_check(ops, x, gamma, f"rmsnorm C {C} rows {rows} vae_rms3 {rms3}", lambda s: ops.vae_rmsnorm_silu(xd, gd, silu=s).cpu())
        if C in (192, 384):
            def padded(s):
                parent = _nan((1 + 2 + 1 + 1, 3, rows + 2, C))
                buf = parent[1:4]
                buf.zero_()
                buf[:2, 1, 1:rows + 1] = 3.0
                view = ops.vae_rmsnorm_silu_padded(xd.view(1, 1, rows, C), gd, buf, silu=s)
                assert float(buf[:, 0].float().abs().sum()) == 0 and float(buf[:, 2].float().abs().sum()) == 0 and float(buf[:, :, 0].float().abs().sum()) == 0
                assert float(buf[:, :, rows + 1].float().abs().sum()) == 0 and bool((buf[:2, 1, 1:rows + 1] == 3).all()) and bool(torch.isnan(parent[4].float()).all())
                return view.reshape(rows, C).cpu()
            _rms_check(ops, x, gamma, f"rmsnorm padded C {C} rows {rows}", padded)


def test_rmsnorm_silu_past_the_grid_cap(ops):
    """65541 rows of 264 channels (64 lanes per row: 4096 workgroups x 4 rows x 4 row groups = 65536 rows per trip): the grid-stride
    loop takes a second trip."""
    rows, C = V.RMS_BIG
    x, gamma = V.rms_inputs(rows, C)
    xd, gd = x.cuda(), gamma.cuda()
    _rms_check(ops, x, gamma, f"rmsnorm C {C} rows {rows}", lambda s: ops.vae_rmsnorm_silu(xd, gd, silu=s).cpu())


# ---------------------------------------------------------------------------------------------------------------------
# softmax rows
@pytest.mark.parametrize("ncols", V.SOFTMAX_NCOLS)
def test_softmax_rows_within_the_derived_bound(ops, ncols):
    """gf_softmax_rows: nvalid 1 / ncols - 1 / ncols, with and without a bias, x and bias as column slices of NaN-filled parents
    (ldx = ncols + 8, ldb = ncols + 16), the masked columns holding 1e30, ldo = ncols rounded up to 64 with the pad exactly zero."""
    ldo = -(-ncols // 64) * 64
    for nc, nv, with_bias, std in V.softmax_cases():
        if nc != ncols:
            continue
        x, scale, bias = V.softmax_inputs(nc, nv, with_bias, std)
        px = _nan((x.shape[0], nc + 8))
        px[:, :nc] = x.cuda()
        pb = None
        if bias is not None:
            pb = _nan((x.shape[0], nc + 16))
            pb[:, :nc] = bias.cuda()
        got = ops.softmax_rows(px[:, :nc], scale, ldo, bias=None if pb is None else pb[:, :nc], nvalid=nv).cpu()
        p, bound = V.softmax_rows_chain(x, scale, bias, nv, ldo)
        outside, worst, pad0 = V.softmax_judge(got, p, bound)
        print(f"PIN softmax_rows ncols {nc} nvalid {nv} bias {with_bias} std {std:g}: {outside} outside, worst {worst:.3f} of the bound, row sums "
              f"{float(got.double().sum(-1).min()):.4f} .. {float(got.double().sum(-1).max()):.4f}")
        assert outside == 0, f"softmax ncols {nc} nvalid {nv} bias {with_bias} std {std}: {outside} elements outside the bound (worst {worst:.2f}x)"
        assert pad0, f"softmax ncols {nc} nvalid {nv}: columns from nvalid to ldo are not exactly zero"
        f = FIG.setdefault("softmax_rows", dict(cases=0, worst=0.0))
        f["cases"] += 1
        f["worst"] = max(f["worst"], worst)


# ---------------------------------------------------------------------------------------------------------------------
# the latent scale steps
def _latent_stats(g):
    mean = torch.randn(16, generator=g).to(BF)
    inv_std = (1.0 / (0.5 + 2.5 * torch.rand(16, generator=g))).to(BF)
    return mean, inv_std


def test_prep_latent_bit_for_bit(ops):
    """A strided tile slice of a larger NaN-filled latent, C = 16 into cpad = 64: bf16(bf16(z / inv_std) + mean) bit for bit (the
    division and the add are single IEEE operations), the pad channels exactly zero."""
    g = torch.Generator().manual_seed(21)
    mean, inv_std = _latent_stats(g)
    z = (torch.randn((16, 3, 6, 8), generator=g) * 1.5).to(BF)
    z[:, 0, 0, :3] = torch.tensor([0.0, -0.0, 1e30]).to(BF)
    big = _nan((20, 5, 12, 14))
    big[2:18, 1:4, 3:9, 2:10] = z.cuda()
    got = ops.vae_prep_latent(big[2:18, 1:4, 3:9, 2:10], mean.cuda(), inv_std.cuda(), cpad=64).cpu()
    want = V.prep_latent_ref(z, mean, inv_std, 64)
    diff = _bits(got) != _bits(want)
    print(f"PIN prep_latent: {int(diff.sum())} of {diff.numel()} differ from the fp32 formula")
    assert not bool(diff.any()), f"{int(diff.sum())} elements differ; worst {int(R.bf16_steps(got, want).max())} bf16 steps"
    assert bool((_bits(got[..., 16:]) == 0).all())


def test_finish_latent_bit_for_bit(ops):
    """The encoder tail on the first 16 of 32 conv1 channels, rows as a column slice (ldx = 40) of a NaN-filled parent."""
    g = torch.Generator().manual_seed(22)
    mean, inv_std = _latent_stats(g)
    for rows in (1, 255, 4099):
        x = (torch.randn((rows, 32), generator=g) * 2).to(BF)
        par = _nan((rows, 40))
        par[:, :32] = x.cuda()
        got = ops.vae_finish_latent(par[:, :32], mean.cuda(), inv_std.cuda(), 16).cpu()
        want = V.finish_latent_ref(x, mean, inv_std, 16)
        diff = _bits(got) != _bits(want)
        print(f"PIN finish_latent rows {rows}: {int(diff.sum())} of {diff.numel()} differ from the fp32 formula")
        assert got.shape == (rows, 16) and not bool(diff.any()), f"rows {rows}: {int(diff.sum())} elements differ"


def test_print_figures():
    """The figures the docstrings and COVERAGE.md quote (`pytest -s`)."""
    for form, f in sorted(FIG.items()):
        if "row" in f:
            print(f"FIG {form}: {f['cases']} gauss comparisons, worst share {f['share']:.3g}, worst ratio of (b) {f['worst']:.3f}, worst row {f['row'][0]} of cap "
                  f"{f['row'][1]}, worst column {f['col'][0]} of cap {f['col'][1]}")
        else:
            print(f"FIG {form}: {f}")
