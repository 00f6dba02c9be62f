"""MXFP4 linears on the device (goal_force_amd/csrc/gf_gemm_mxfp4.hip: gf_quant_mxfp4, gf_gemm_mxfp4; dit.enable_fp4) against the
restatements of tests/fp4_refs.py:

  quantiser   codes and scales torch.equal with fp4_refs.quantize on Gaussians at three scales, every bf16 value (once the maximum of its
              block, once beside a larger element), zero blocks and non-finite entries; strided rows inside NaN parents, outputs inside
              0xFF parents with the guards intact;
  layout      one-hot rows of A, asymmetric W, a distinct scale exponent in every block of A and of W: one nonzero product per output,
              exact whatever the accumulator does — the nibble order, the k order inside a lane, which lane supplies which block's scale
              and what opsel selects;
  integers    e2m1-grid values and power-of-two scales with exact fp32 sums: torch.equal with the chain (epilogues 1, 4: gf_act of it);
  gauss       the two bars of gemm_refs.judge against the exact chain on the DEQUANTISED operands — the GEMM is judged on what it was
              given; quantisation error is not its business — at every tile edge and epilogue;
  NaN scales, memory discipline, refusals by message, and the module switch against the same block with the named Linears restated in
  fp64 from fake-quantised inputs and weights.
The guarantees checked are the mechanism's: no test here makes a quality claim.

Measured on an MI355X (`pytest -s` prints every comparison; profiles/r15/test_fp4_gpu_figures.log):
  quantiser, layout, integers   equal everywhere.
  gauss class                   78 comparisons + the memory-discipline cases: 0 differing bf16 bits against the chain on the model's
                                accumulator (cap 2^-10) and against the exact chain alike; worst ratio of bar (b) 0 — on operands from
                                the quantiser every output equalled bf16(exact chain).
  model, random codes / scales  scale ranges 2^+-0, 2^+-3, 2^+-4: equal to bf16(model).  2^+-8 at K = 1280: 5.8e-5 of the outputs differ
                                from the model (1.2e-4 from the exact product); 2^+-30: 1.2e-3 (1.5e-3).  Worst |got - exact| over
                                2^-8 |exact| + K 2^-23 S + T: 0.97 (the bf16 rounding).
No model reproduces the instruction's bits over wide scale ranges (fp4_refs.MODEL_NOTE): bar (a) is held against the closest model and
bar (b) against the exact chain with the bound T derived from that model's worst case.
"""
import pytest
import torch

import fp4_refs as F
import gemm_refs as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U8 = torch.uint8
SENT = 0x5A5A                       # a finite bf16 bit pattern (1.5e16) no output here comes near
GF_ERR_INVALID_ARG = -1
NEED_R = (R.EPI_GATE_RESID, R.EPI_RESID, R.EPI_MUL)
KINDS = {R.EPI_GELU: "gelu_tanh", R.EPI_SILU: "silu"}
FIG = {}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from goal_force_amd import ops as _ops
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


_CACHE = {}


def _ptr(t):
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _sentinel(shape):
    t = torch.empty(shape, dtype=BF, device="cuda")
    t.view(torch.int16).fill_(SENT)
    return t


def _intact(t):
    return bool((t.view(torch.int16) == SENT).all())


def _in_ff_parent(t, cols_before=16, cols_after=16, rows_after=3):
    """A uint8 [rows, cols] tensor as a column slice of a parent filled with 0xFF (the NaN scale; in an operand, -6 in both nibbles)."""
    rows, cols = t.shape
    par = torch.full((rows + rows_after, cols_before + cols + cols_after), 0xFF, dtype=U8, device="cuda")
    par[:rows, cols_before:cols_before + cols] = t
    return par[:rows, cols_before:cols_before + cols], par


# ---------------------------------------------------------------------------------------------------------------------
# the quantiser
def _every_bf16_value():
    """[65536, 64]: block 0 holds value v alone (v is the maximum), block 1 holds v beside a finite element of at least its magnitude."""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)
    x = torch.zeros((65536, 64), dtype=BF)
    x[:, 5] = v
    x[:, 32 + 9] = v
    big = (v.float().abs() * 4).clamp(max=3.3895e38).to(BF)
    x[:, 32 + 20] = torch.where(torch.isfinite(v.float()), big, torch.ones_like(big))
    return x


def _quant_class(cls, rows, dim):
    g = torch.Generator().manual_seed(rows * 100003 + dim)
    if cls.startswith("gauss"):
        return (torch.randn((rows, dim), generator=g) * float(cls[5:])).to(BF)
    if cls == "zeros_and_nonfinite":
        x = torch.randn((rows, dim), generator=g).to(BF)
        nb = dim // 32
        for r in range(rows):
            x[r, 32 * (r % nb):32 * (r % nb) + 32] = 0.0                                   # a zero block per row
            if r % 3 == 0:
                x[r, (7 * r + 40) % dim] = (float("nan"), float("inf"), float("-inf"))[(r // 3) % 3]
        x[rows // 2] = -0.0
        return x
    raise AssertionError(cls)


QUANT_CASES = [(1, 32, "gauss1"), (7, 64, "gauss1e-3"), (64, 256, "gauss1e3"), (65, 1536, "zeros_and_nonfinite"), (513, 5120, "gauss1"),
               (7, 13824, "gauss1e3"), (513, 32, "zeros_and_nonfinite"), (1, 13824, "gauss1e-3"), (65, 64, "gauss1"), (64, 5120, "zeros_and_nonfinite"),
               (513, 256, "gauss1e-3"), (7, 1536, "gauss1")]


@pytest.mark.parametrize("rows,dim,cls", QUANT_CASES)
def test_quantiser_equals_the_restatement(ops, rows, dim, cls):
    """Strided rows inside a NaN parent: a read outside the rows would turn a block's scale into 255."""
    x = _quant_class(cls, rows, dim)
    par = torch.full((rows + 2, dim + 16), float("nan"), dtype=BF, device="cuda")
    par[:rows, 8:8 + dim] = x.cuda()
    x4, sc = ops.quant_mxfp4(par[:rows, 8:8 + dim])
    r4, rs = F.quantize(x)
    assert torch.equal(sc.cpu(), rs), f"scales differ at {torch.nonzero(sc.cpu() != rs)[:4].tolist()}"
    assert torch.equal(x4.cpu(), r4), f"codes differ at {torch.nonzero(x4.cpu() != r4)[:4].tolist()}"


def test_quantiser_on_every_bf16_value(ops):
    x = _every_bf16_value()
    x4, sc = ops.quant_mxfp4(x.cuda())
    r4, rs = F.quantize(x)
    assert torch.equal(sc.cpu(), rs), f"scales differ at rows {torch.nonzero(sc.cpu() != rs)[:4].tolist()}"
    assert torch.equal(x4.cpu(), r4), f"codes differ at {torch.nonzero(x4.cpu() != r4)[:4].tolist()}"


def test_quantiser_writes_only_its_outputs_and_takes_no_rows(ops, lib):
    rows, dim = 65, 256
    x = _quant_class("gauss1", rows, dim).cuda()
    z4 = torch.zeros((rows, dim // 2), dtype=U8, device="cuda")
    zs = torch.zeros((rows, dim // 32), dtype=U8, device="cuda")
    (o4, p4), (os_, ps) = _in_ff_parent(z4), _in_ff_parent(zs, 5, 3)          # the scale rows start at an odd address and stride
    rc = lib.gf_quant_mxfp4(_ptr(x), x.stride(0), _ptr(o4), o4.stride(0), _ptr(os_), os_.stride(0), rows, dim, _st())
    torch.cuda.synchronize()
    assert rc == 0
    r4, rs = F.quantize(x.cpu())
    assert torch.equal(o4.cpu(), r4) and torch.equal(os_.cpu(), rs)
    for par, view, before in ((p4, o4, 16), (ps, os_, 5)):
        guard = par.clone()
        guard[:rows, before:before + view.shape[1]] = 0xFF
        assert bool((guard == 0xFF).all()), "the quantiser wrote outside its outputs"
    p4.fill_(0xFF)
    assert lib.gf_quant_mxfp4(_ptr(x), x.stride(0), _ptr(o4), o4.stride(0), _ptr(os_), os_.stride(0), 0, dim, _st()) == 0
    torch.cuda.synchronize()
    assert bool((p4 == 0xFF).all())
    for bad_dim, bad_stride in ((48, dim), (dim, dim // 2 - 4)):
        rc = lib.gf_quant_mxfp4(_ptr(x), x.stride(0), _ptr(o4), bad_stride if bad_dim == dim else o4.stride(0), _ptr(os_), os_.stride(0), rows, bad_dim, _st())
        assert rc == GF_ERR_INVALID_ARG and b"gf_quant_mxfp4" in lib.gf_last_error()
    torch.cuda.synchronize()
    assert bool((p4 == 0xFF).all())


# ---------------------------------------------------------------------------------------------------------------------
# the GEMM: cases, computed once and left unchanged
CLASSES = dict(gauss=F.gauss_inputs, integers=F.integer_inputs, selector=F.selector_inputs)


def _case(ops, cls, M, N, K, seed=0):
    key = (cls, M, N, K, seed)
    if key not in _CACHE:
        d = CLASSES[cls](M, N, K, seed=seed)
        if cls == "gauss":                # the operands the product path feeds the kernel: the device's own quantiser
            for x, p, s in ((d["x"], "a4", "sa"), (d["w_bf16"], "w4", "sw")):
                q4, qs = ops.quant_mxfp4(x.cuda())
                assert torch.equal(q4.cpu(), d[p]) and torch.equal(qs.cpu(), d[s]), f"gauss {M} x {N} x {K}: the device quantiser departs from fp4_refs.quantize"
        dev = {k: d[k].cuda() for k in ("a4", "sa", "w4", "sw", "bias", "resid", "gate")}
        _CACHE[key] = dict(d=d, dev=dev, ref={}, cls=cls, shape=(M, N, K))
    return _CACHE[key]


def _ref(case, epi):
    if epi not in case["ref"]:
        case["ref"][epi] = F.reference(case["d"], epi)
    return case["ref"][epi]


def _run(ops, case, epi, bias=True):
    v = case["dev"]
    return ops.gemm_mxfp4(v["a4"], v["sa"], v["w4"], v["sw"], v["bias"] if bias else None, epilogue=epi, resid=v["resid"] if epi in NEED_R else None,
                          gate=v["gate"] if epi == R.EPI_GATE_RESID else None).cpu()


def _act_of(ops, y, epi):
    """gf_act on the exact bf16 Linear (the epilogue's -0 on the header's two tail ranges restated)."""
    out = ops.act(y.cuda().contiguous(), KINDS[epi]).cpu()
    return torch.where(R.tail_mask(y, epi), torch.full_like(out, -0.0), out)


def _check_exact(ops, case, epi, what):
    r = _ref(case, epi)
    got = _run(ops, case, epi)
    if epi in KINDS:
        want = _act_of(ops, _ref(case, R.EPI_BIAS).out.to(BF), epi)
    else:
        want = r.out.to(BF)
    bad = torch.nonzero(_bits(got) != _bits(want))
    assert bad.numel() == 0, f"{what} epilogue {R.EPI_NAMES[epi]}: {bad.shape[0]} of {got.numel()} differ, first (row, column) {bad[:4].tolist()}: " \
                             f"got {[float(got[i, j]) for i, j in bad[:4].tolist()]} want {[float(want[i, j]) for i, j in bad[:4].tolist()]}"


LAYOUT_SHAPES = [(513, 264, 512), (257, 56, 256), (17, 8, 1280), (513, 520, 768)]


@pytest.mark.parametrize("M,N,K", LAYOUT_SHAPES)
def test_layout_one_product_per_output(ops, M, N, K):
    """f(m) = m mod K at M = 513 takes every one of the 256 positions of a K tile in both tile parities (K = 512) and in three tiles
    (K = 768)."""
    case = _case(ops, "selector", M, N, K)
    d = case["d"]
    if M >= K:
        assert set(d["k"].tolist()) == set(range(K))
    v = case["dev"]
    got = ops.gemm_mxfp4(v["a4"], v["sa"], v["w4"], v["sw"]).cpu()
    acc, _ = F.product(*F.operands(d))
    want = acc.to(BF)
    assert torch.equal(acc, want.double()), "one product of two e2m1 values and two powers of two is a bf16 value"
    assert len({int(s) for s in d["sa"][0]}) == K // 32 and len({int(s) for s in d["sw"][0]}) == K // 32
    bad = torch.nonzero(_bits(got) != _bits(want))
    assert bad.numel() == 0, f"{bad.shape[0]} of {got.numel()} differ; first (row, column, k): {[(i, j, int(d['k'][i])) for i, j in bad[:6].tolist()]}"


@pytest.mark.parametrize("epi", R.EPIS)
@pytest.mark.parametrize("M,N,K", [(257, 264, 768), (513, 520, 256), (17, 56, 1280)])
def test_integer_class_is_exact(ops, M, N, K, epi):
    _check_exact(ops, _case(ops, "integers", M, N, K), epi, f"integers {M} x {N} x {K}")


def _pinned(ops, case, epi, what, bias=True):
    r = _ref(case, epi)
    if not bias:
        d = dict(case["d"], bias=None)
        d.pop("_mfma", None)
        r = F.reference(d, epi)
    j = R.assert_pinned(_run(ops, case, epi, bias), r, case["shape"][2], what)
    f = FIG.setdefault("gauss", dict(n=0, share=0.0, worst=0.0, share_exact=0.0))
    f["n"] += 1
    for k in ("share", "worst", "share_exact"):
        f[k] = max(f[k], j[k])
    return j


@pytest.mark.parametrize("M,N,K", F.SHAPES)
def test_gauss_class_at_every_tile_edge(ops, M, N, K):
    case = _case(ops, "gauss", M, N, K)
    for epi in R.EPIS:
        _pinned(ops, case, epi, f"mxfp4 gauss {M} x {N} x {K} {R.EPI_NAMES[epi]}")


def test_mfma_model_on_random_codes_and_scales(ops):
    """What fp4_refs.mfma_mxfp4 says of the instruction, held the way test_fp8_mfma_model holds the fp8 model: random codes over all 16
    and random scales, no bias.  Where zero differences were measured (block scales within 2^+-4 per operand) the kernel returns
    bf16(the model's accumulator); over wide exponent ranges the model is only the closest one (fp4_refs.MODEL_NOTE) and what is held is
    the derived bound: |kernel - exact product| <= 2^-8 |exact| + K 2^-23 S + T."""
    g = torch.Generator().manual_seed(11)
    for (M, N, K, delta, equal) in ((64, 64, 256, 0, True), (64, 64, 256, 4, True), (513, 520, 512, 3, True), (64, 64, 512, 30, False), (130, 264, 1280, 8, False)):
        A, W = F._rand_codes((M, K), g), F._rand_codes((N, K), g)
        sa = (127 + torch.randint(-delta, delta + 1, (M, K // 32), generator=g)).to(U8)
        sw = (127 + torch.randint(-delta, delta + 1, (N, K // 32), generator=g)).to(U8)
        a4, w4 = F.pack(A), F.pack(W)
        got = ops.gemm_mxfp4(a4.cuda(), sa.cuda(), w4.cuda(), sw.cuda()).cpu()
        acc_m, T = F.mfma_mxfp4(a4, sa, w4, sw)
        exact, S = F.product(a4, sa, w4, sw)
        model = float((_bits(got) != _bits(acc_m.to(BF))).double().mean())
        plain = float((_bits(got) != _bits(exact.to(BF))).double().mean())
        allow = 2.0 ** -8 * exact.abs() + K * R.ULP32 * S + T
        ratio = float(((got.double() - exact).abs() / allow.clamp_min(1e-300)).max())
        print(f"PIN mxfp4 MFMA model {M} x {N} x {K}, scales 2^+-{delta}: bits differ from bf16(model) on {model:.2e} of the elements, from "
              f"bf16(exact product) on {plain:.2e}; worst |got - exact| / (2^-8 |exact| + K 2^-23 S + T) = {ratio:.3f}")
        assert ratio <= 1.0, (M, N, K, delta, ratio)
        assert model == 0.0 or not equal, (M, N, K, delta, model)


# ---------------------------------------------------------------------------------------------------------------------
# NaN scales
def test_nan_scale_rows_and_columns(ops):
    M, N, K = 257, 264, 768
    case = _case(ops, "gauss", M, N, K)
    v = case["dev"]
    for epi in R.EPIS:
        sa, sw = v["sa"].clone(), v["sw"].clone()
        sa[5, 3], sa[256, 23], sw[9, 20], sw[263, 0] = 255, 255, 255, 255
        got = ops.gemm_mxfp4(v["a4"], sa, v["w4"], sw, v["bias"], epilogue=epi, resid=v["resid"] if epi in NEED_R else None,
                             gate=v["gate"] if epi == R.EPI_GATE_RESID else None).cpu()
        nan = torch.isnan(got)
        want = torch.zeros_like(nan)
        want[[5, 256]] = True
        want[:, [9, 263]] = True
        assert torch.equal(nan, want), f"epilogue {R.EPI_NAMES[epi]}: NaN at {int(nan.sum())} elements, expected rows 5, 256 and columns 9, 263 ({int(want.sum())})"
        clean = _run(ops, case, epi)
        assert torch.equal(_bits(got)[~want], _bits(clean)[~want]), "a NaN scale changed an element outside its row / column"
    # the quantiser's NaN block reaches the output the same way
    x = case["d"]["x"].clone()
    x[7, 300] = float("inf")
    a4, sa = ops.quant_mxfp4(x.cuda())
    got = ops.gemm_mxfp4(a4, sa, v["w4"], v["sw"], v["bias"]).cpu()
    assert bool(torch.isnan(got[7]).all()) and int(torch.isnan(got).sum()) == N


# ---------------------------------------------------------------------------------------------------------------------
# memory discipline, through the raw ABI
def _raw(lib, A, lda, sa, lsa, W, ldw, sw, lsw, bias, C, ldc, M, N, K, epi, resid, ldr, gate):
    rc = lib.gf_gemm_mxfp4(_ptr(A), lda, _ptr(sa), lsa, _ptr(W), ldw, _ptr(sw), lsw, _ptr(bias), _ptr(C), ldc, M, N, K, epi, _ptr(resid), ldr,
                           _ptr(gate), _st())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("M,N,K", [(257, 264, 768), (17, 520, 256)])
def test_ff_surroundings_guards_aliasing_null_bias_and_no_rows(ops, lib, M, N, K):
    """Operands and scale arrays inside 0xFF parents (0xFF is the NaN scale: any over-read of a scale row poisons an output, and an
    over-read operand row is -6 in every element), C with ldc = N + 8 between sentinels, C aliasing resid, bias = NULL, M = 0."""
    case = _case(ops, "gauss", M, N, K)
    v = case["dev"]
    (a4, _), (w4, _) = _in_ff_parent(v["a4"], 16, 16), _in_ff_parent(v["w4"], 32, 16)
    (sa, _), (sw, _) = _in_ff_parent(v["sa"], 3, 5), _in_ff_parent(v["sw"], 1, 2)
    for epi in R.EPIS:
        r = _ref(case, epi)
        cpar = _sentinel((M + 2, N + 8))
        C = cpar[1:1 + M, :N]
        resid = v["resid"] if epi in NEED_R else None
        rc = _raw(lib, a4, a4.stride(0), sa, sa.stride(0), w4, w4.stride(0), sw, sw.stride(0), v["bias"], C, N + 8, M, N, K, epi, resid, N,
                  v["gate"] if epi == R.EPI_GATE_RESID else None)
        assert rc == 0, lib.gf_last_error()
        got = C.cpu()
        assert not bool(torch.isnan(got).any()), "a NaN reached the output: an operand or a scale was read outside its rows"
        assert _same(got, _run(ops, case, epi)), f"epilogue {epi}: strided operands in 0xFF parents change the result"
        assert _intact(cpar[0]) and _intact(cpar[1 + M]) and _intact(cpar[1:1 + M, N:]), "a store outside C"
        R.assert_pinned(got, r, K, f"mxfp4 in 0xFF parents {M} x {N} x {K} {R.EPI_NAMES[epi]}")
        if epi in NEED_R:                      # C aliases resid
            buf = v["resid"].clone()
            rc = _raw(lib, a4, a4.stride(0), sa, sa.stride(0), w4, w4.stride(0), sw, sw.stride(0), v["bias"], buf, N, M, N, K, epi, buf, N,
                      v["gate"] if epi == R.EPI_GATE_RESID else None)
            assert rc == 0 and _same(buf.cpu(), got), f"epilogue {epi}: C aliasing resid changes the result"
    # bias = NULL behaves as a zero bias
    zero = torch.zeros(N, dtype=BF, device="cuda")
    for epi in (R.EPI_BIAS, R.EPI_GELU, R.EPI_GATE_RESID):
        kw = dict(epilogue=epi, resid=v["resid"] if epi in NEED_R else None, gate=v["gate"] if epi == R.EPI_GATE_RESID else None)
        assert _same(ops.gemm_mxfp4(v["a4"], v["sa"], v["w4"], v["sw"], None, **kw).cpu(), ops.gemm_mxfp4(v["a4"], v["sa"], v["w4"], v["sw"], zero, **kw).cpu())
    _pinned(ops, case, R.EPI_BIAS, f"mxfp4 no bias {M} x {N} x {K}", bias=False)
    # M = 0: nothing is launched, nothing is written
    cpar = _sentinel((2, N))
    assert _raw(lib, a4, a4.stride(0), sa, sa.stride(0), w4, w4.stride(0), sw, sw.stride(0), v["bias"], cpar, N, 0, N, K, 0, None, 0, None) == 0
    assert _intact(cpar)
    assert tuple(ops.gemm_mxfp4(v["a4"][:0], v["sa"][:0], v["w4"], v["sw"]).shape) == (0, N)


def test_refusals_by_message_with_outputs_untouched(ops, lib):
    M, N, K = 17, 56, 512
    case = _case(ops, "gauss", M, N, K)
    v = case["dev"]
    a4, sa, w4, sw = v["a4"], v["sa"], v["w4"], v["sw"]
    C = _sentinel((M, N))
    ok = dict(A=a4, lda=K // 2, sa=sa, lsa=K // 32, W=w4, ldw=K // 2, sw=sw, lsw=K // 32, bias=v["bias"], C=C, ldc=N, M=M, N=N, K=K, epi=0,
              resid=v["resid"], ldr=N, gate=v["gate"])
    cases = [
        (dict(A=None), "null A/W/C/scales"), (dict(W=None), "null A/W/C/scales"), (dict(C=None), "null A/W/C/scales"),
        (dict(sa=None), "null A/W/C/scales"), (dict(sw=None), "null A/W/C/scales"),
        (dict(epi=6), "unknown epilogue 6"), (dict(epi=-1), "unknown epilogue -1"),
        (dict(epi=2, resid=None), "residual epilogue needs an aligned resid"), (dict(epi=3, resid=None), "residual epilogue needs an aligned resid"),
        (dict(epi=5, ldr=N - 8), "residual epilogue needs an aligned resid"), (dict(epi=2, gate=None), "gate epilogue needs an aligned gate vector"),
        (dict(K=K - 128), "K=384 must be a multiple of 256"), (dict(K=K - 32), "K=480 must be a multiple of 256"), (dict(K=0), "bad sizes"),
        (dict(N=N - 4), "N=52 must be a multiple of 8"), (dict(M=-1), "bad sizes"),
        (dict(lda=K // 2 + 8), "leading dimensions must be multiples of 16"), (dict(ldw=K // 2 - 16), "leading dimensions must be multiples of 16"),
        (dict(ldc=N + 4), "leading dimensions must be multiples of 16"), (dict(ldc=N - 8), "leading dimensions must be multiples of 16"),
        (dict(lsa=K // 32 - 1), "scale strides must cover K/32 = 16 blocks"), (dict(lsw=0), "scale strides must cover K/32 = 16 blocks"),
        (dict(A=a4.data_ptr() + 8), "16-byte alignment required"), (dict(bias=v["bias"].data_ptr() + 2), "16-byte alignment required"),
        (dict(M=1 << 30), "M/N too large"), (dict(lda=1 << 24), "operand too large for 32-bit staging offsets"),
        (dict(lsw=1 << 24), "operand too large for 32-bit staging offsets"),
    ]
    for change, msg in cases:
        a = dict(ok, **change)
        rc = _raw(lib, a["A"], a["lda"], a["sa"], a["lsa"], a["W"], a["ldw"], a["sw"], a["lsw"], a["bias"], a["C"], a["ldc"], a["M"], a["N"], a["K"],
                  a["epi"], a["resid"], a["ldr"], a["gate"])
        err = lib.gf_last_error().decode()
        assert rc == GF_ERR_INVALID_ARG and err.startswith("gf_gemm_mxfp4: ") and msg in err, (change, rc, err)
        assert _intact(C), f"{change}: a refused call wrote to C"
    # the wrapper's own vocabulary
    from goal_force_amd._lib import GoalForceError
    for kw, msg in ((dict(a4=a4.view(torch.int8)), "expected dtype torch.uint8"), (dict(a_scale=sa[:, :-1]), "activation scales: expected"),
                    (dict(w_scale=None), "weight scales: required"), (dict(w4=w4[:, :-16]), "weight: expected"), (dict(out=C[:, :-8]), "gemm_mxfp4.out: expected"),
                    (dict(epilogue=3, resid=v["resid"][:-1]), "gemm_mxfp4.resid: expected"), (dict(bias=v["bias"][:-8]), "gemm_mxfp4.bias: expected contiguous"),
                    (dict(a4=a4.cpu()), "must be on the GPU")):
        args = dict(dict(a4=a4, a_scale=sa, w4=w4, w_scale=sw, bias=v["bias"], out=C), **kw)
        with pytest.raises(GoalForceError, match=msg):
            ops.gemm_mxfp4(**args)
    with pytest.raises(GoalForceError, match="multiple of 32"):
        ops.quant_mxfp4(torch.zeros((4, 48), dtype=BF, device="cuda"))
    torch.cuda.synchronize()
    assert _intact(C)


# ---------------------------------------------------------------------------------------------------------------------
# the module switch
DIM, HEADS, FFN, S, CTX = 256, 2, 512, 300, 64
GRID = (3, 10, 10)


def _block_and_inputs():
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    import gen_inputs as gi
    from goal_force_amd.dit import DiTBlock, RopeTable, precompute_freqs_cis_3d
    sd = gi.block_sd(torch.Generator().manual_seed(61), DIM, FFN, "", BF)
    x, ctx, t_mod = gi.block_inputs(DIM, S, CTX, seed=62)
    blk = DiTBlock(False, DIM, HEADS, FFN, 1e-6)
    blk.load_state_dict(sd, strict=True)
    rope = RopeTable.from_grid(precompute_freqs_cis_3d(128), *GRID, "cuda")
    return blk.to(BF).cuda(), (x.cuda(), ctx.cuda(), t_mod.cuda(), rope)


def _restated_linear(dit, real):
    """dit.linear with every enable_fp4 layer restated: fp64 product of the fake-quantised input and weight (fp4_refs.fake_quant), then
    the epilogue's chain (gemm_refs.chain) — every other layer goes to the real function."""
    def linear(x2, lin, epilogue=0, resid=None, gate=None, out=None):
        if getattr(lin, "_gf_w4", None) is None:
            return real(x2, lin, epilogue=epilogue, resid=resid, gate=gate, out=out)
        assert x2.dtype == BF, "an enable_fp4 layer is handed bf16"
        acc = F.fake_quant(x2.cpu()) @ F.fake_quant(lin.weight.detach().cpu()).t()
        y = R.chain(acc, lin.bias.detach().cpu(), int(epilogue), None if resid is None else resid.cpu(), None if gate is None else gate.cpu())[0]
        y = y.to(BF).cuda()
        return y if out is None else out.copy_(y)
    return linear


@pytest.mark.parametrize("layers", [("ffn",), ("o",), ("ffn", "o")])
@pytest.mark.parametrize("fp8", [False, True])
def test_block_under_enable_fp4_equals_its_restatement(monkeypatch, layers, fp8):
    from goal_force_amd import dit
    blk, inputs = _block_and_inputs()
    before = blk(*inputs).clone()
    if fp8:
        dit.enable_fp8(blk)
        before8 = blk(*inputs).clone()
    dit.enable_fp4(blk, layers=layers)
    named = {"ffn": ["ffn.0", "ffn.2"], "o": ["self_attn.o", "cross_attn.o"]}
    assert sorted(n for n, m in blk.named_modules() if getattr(m, "_gf_w4", None) is not None) == sorted(sum((named[x] for x in layers), []))
    got = blk(*inputs).clone()
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, before8 if fp8 else before)
    monkeypatch.setattr(dit, "linear", _restated_linear(dit, dit.linear))
    ref = blk(*inputs).clone()
    monkeypatch.undo()
    e = float((got.float() - ref.float()).norm() / ref.float().norm())
    print(f"PIN enable_fp4 block layers={layers} fp8={fp8}: rel-L2 to the restated block {e:.3e}")
    assert e < 5e-3, f"rel-L2 {e:.3e}"
    # off again: the bits the block had before
    dit.enable_fp4(blk, False)
    assert torch.equal(blk(*inputs), before8 if fp8 else before)
    if fp8:
        dit.enable_fp8(blk, False)
        assert torch.equal(blk(*inputs), before)


def test_an_fp8_input_to_an_fp4_layer_and_training_are_refused():
    from goal_force_amd import dit
    from goal_force_amd._lib import GoalForceError
    blk, inputs = _block_and_inputs()
    dit.enable_fp4(blk)
    q = dit.QuantizedInput(inputs[0][0])
    with pytest.raises(GoalForceError, match="QuantizedInput"):
        dit.linear(q, blk.ffn[0])
    with pytest.raises(GoalForceError, match="training through an enable_fp4 block is refused"):
        dit.refuse_training(blk)


def test_pipeline_level_switch_runs_and_is_finite():
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    import gen_inputs as gi
    from goal_force_amd import dit
    from goal_force_amd.controlnet import ControlNet
    from goal_force_amd.model_fn import model_fn_wan_video
    cfg = gi.TINY
    model = dit.WanModel(has_image_input=False, require_clip_embedding=False, **cfg)
    model.load_state_dict(gi.dit_sd(cfg, seed=41), strict=True)
    cn = ControlNet(gi.TINY_CONTROLNET_LAYERS, dim=cfg["dim"], num_heads=cfg["num_heads"], ffn_dim=cfg["ffn_dim"])
    cn.load_state_dict(gi.controlnet_sd(cfg, gi.TINY_CONTROLNET_LAYERS, seed=42, zero_convs_zero=False), strict=True)

    class Pipe(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.dit, self.controlnet = model.to(BF).cuda(), cn.to(BF).cuda()

    pipe = Pipe()
    inp = {k: v.cuda() for k, v in gi.tiny_inputs().items()}
    ts = torch.tensor([995.9], dtype=BF).cuda()

    def forward():
        return model_fn_wan_video(pipe.dit, latents=inp["latents"], timestep=ts, context=inp["ctx_posi"], y=inp["y"], controlnet=pipe.controlnet,
                                  control_signal_video_latents=inp["control"], elide_zero_controlnet=False).clone()

    base = forward()
    dit.enable_fp4(pipe)
    n4 = sum(getattr(m, "_gf_w4", None) is not None for m in pipe.modules())
    assert n4 == 4 * (cfg["num_layers"] + gi.TINY_CONTROLNET_LAYERS)
    out = forward()
    assert bool(torch.isfinite(out).all()) and not torch.equal(out, base)
    dit.enable_fp4(pipe, False)
    assert torch.equal(forward(), base)


def test_zz_figures():
    """Prints what the gauss comparisons of this run measured (pytest -s)."""
    for k, f in FIG.items():
        print(f"FIG mxfp4 {k}: {f['n']} comparisons, worst share of differing bits {f['share']:.3e} (cap {R.SHARE_CAP:.3e}), worst ratio of bar (b) "
              f"{f['worst']:.3f}, worst share against the exact chain {f['share_exact']:.3e}")
