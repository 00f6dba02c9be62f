"""The two fused MXFP4 producers on the device — gf_layernorm_modulate_mxfp4 (gf_rowops.hip) and gf_gemm_mxfp4_q4 (gf_gemm_mxfp4.hip) —
and the three-launch FFN of an enable_fp4 block (dit.DiTBlock.forward, ops.options(fp4_fused=...)).

The bar everywhere is torch.equal on codes and on scales against the unfused pair through the public wrappers:
    layernorm_modulate_mxfp4(x, ...)  ==  quant_mxfp4(layernorm_modulate(x, ...))
    gemm_mxfp4_q4(a, w, bias, epi)    ==  quant_mxfp4(gemm_mxfp4(a, w, bias, epi))
The quantiser is integer work on bf16 bit patterns, so quantising the bf16 values the pair would have stored gives the pair's bytes; the
pair itself is pinned elsewhere (the LayerNorm per element by test_forward_kernels_gpu.py, the quantiser and the GEMM by
test_fp4_gpu.py).  With the fused route on, test_fp4_gpu.py's restated block covers only the "o" layers: the FFN's pin against the fp64
restatement lives here (test_block_fused_equals_unfused_and_the_restatement).
"""
import pytest
import torch

import fp4_refs as F
import gemm_refs as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U8 = torch.uint8
GF_ERR_INVALID_ARG = -1
LN_WIDTHS = (1536, 4096, 5120)
LN_ROWS = (1, 3, 4, 5, 9)                 # the edges of 4 rows per workgroup
OPSETS = ((), ("weight", "bias"), ("scale1p", "shift"), ("weight",), ("shift",))      # three on the specialised kernel, two on the nullable one
Q4_SHAPES = [(1, 32, 256), (17, 64, 256), (255, 224, 512), (256, 256, 256), (257, 288, 768), (513, 544, 256), (129, 96, 1280)]
Q4_EPIS = (R.EPI_BIAS, R.EPI_GELU, R.EPI_SILU)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from goal_force_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    return ops._lib.load()


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _ptr(t):
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ff_parent(rows, cols, cols_before, cols_after, rows_after=3):
    """-> (view [rows, cols], parent): a uint8 output as a column slice of a parent filled with 0xFF."""
    par = torch.full((rows + rows_after, cols_before + cols + cols_after), 0xFF, dtype=U8, device="cuda")
    return par[:rows, cols_before:cols_before + cols], par


def _only_the_view_was_written(par, rows, cols_before, cols):
    guard = par.clone()
    guard[:rows, cols_before:cols_before + cols] = 0xFF
    return bool((guard == 0xFF).all())


def _assert_same(got, want, what):
    (g4, gs), (w4, ws) = got, want
    assert g4.shape == w4.shape and gs.shape == ws.shape, (what, g4.shape, w4.shape, gs.shape, ws.shape)
    assert torch.equal(gs, ws), f"{what}: scales differ at {torch.nonzero(gs != ws)[:4].tolist()}"
    assert torch.equal(g4, w4), f"{what}: codes differ at {torch.nonzero(g4 != w4)[:4].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------
# the shared block step
def test_block_step_on_every_bf16_value_under_scales_of_every_range(ops):
    """Every bf16 pattern beside a block maximum 2^k, k from bf16's smallest subnormal to its largest binade: the element coding under scale
    codes 0 (clamped, four ways), 1, 2, 124, 189 and 252 — subnormal elements under the smallest scales, ties, saturation, signed zeros —
    against fp4_refs.quantize.  (A pattern above the maximum, or a non-finite one, sets the block's scale itself: a valid case too.)"""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    maxima = [0x0001, 0x0040] + [(k + 127) << 7 for k in (-126, -125, -124, -123, -1, 64, 127)]       # 2^-133, 2^-127, then normals 2^k
    x = torch.zeros((65536, 32 * len(maxima)), dtype=torch.int16)
    for i, pat in enumerate(maxima):
        x[:, 32 * i + 5] = v
        x[:, 32 * i + 20] = pat
    x = x.view(BF)
    r4, rs = F.quantize(x)
    assert sorted(set(rs[0].tolist())) == [0, 1, 2, 124, 189, 252]
    _assert_same(tuple(t.cpu() for t in ops.quant_mxfp4(x.cuda())), (r4, rs), "every bf16 value under nine block maxima")


# ---------------------------------------------------------------------------------------------------------------------
# the LayerNorm producer
def _strided_in_nan_parent(x):
    """x [rows, dim] as a view with row stride dim + 8 of a NaN-filled parent: a read outside the rows poisons a block."""
    rows, dim = x.shape
    par = torch.full((rows + 1, dim + 8), float("nan"), dtype=BF, device="cuda")
    par[:rows, :dim] = x.cuda()
    return par[:rows, :dim]


def _ln_vectors(dim, g):
    return dict(weight=(1 + 0.1 * torch.randn(dim, generator=g)).to(BF).cuda(), bias=(0.1 * torch.randn(dim, generator=g)).to(BF).cuda(),
                scale1p=(1 + 0.1 * torch.randn(dim, generator=g)).to(BF).cuda(), shift=(0.1 * torch.randn(dim, generator=g)).to(BF).cuda())


def _pair(ops, x, **kw):
    return ops.quant_mxfp4(ops.layernorm_modulate(x, **kw))


@pytest.mark.parametrize("dim", LN_WIDTHS)
def test_layernorm_producer_equals_the_pair(ops, dim):
    g = torch.Generator().manual_seed(dim)
    vec = _ln_vectors(dim, g)
    for rows in LN_ROWS:
        x = _strided_in_nan_parent(torch.randn((rows, dim), generator=g).to(BF))
        assert x.stride(0) == dim + 8
        for names in OPSETS:
            kw = {n: vec[n] for n in names}
            got = ops.layernorm_modulate_mxfp4(x, eps=1e-6, **kw)
            assert got[0].dtype == U8 and tuple(got[0].shape) == (rows, dim // 2) and tuple(got[1].shape) == (rows, dim // 32)
            assert not bool((got[1] == 255).any()), f"dim {dim} rows {rows} {names}: a NaN block: the row was read outside its {dim} columns"
            _assert_same(got, _pair(ops, x, eps=1e-6, **kw), f"dim {dim} rows {rows} operands {names}")


@pytest.mark.parametrize("dim", LN_WIDTHS)
def test_layernorm_producer_on_wide_scales_a_constant_row_and_an_inf(ops, dim):
    g = torch.Generator().manual_seed(7 * dim)
    rows, nb = 9, dim // 32
    # 1 + scale per 32-column block over 2^-40 .. 2^30: block scales of one row 70 binades apart
    expo = torch.linspace(-40, 30, nb).round()
    wide = ((1 + 0.25 * torch.rand(dim, generator=g)) * torch.exp2(expo).repeat_interleave(32)).to(BF).cuda()
    x = torch.randn((rows, dim), generator=g).to(BF)
    x[3] = 0.75                                     # a constant row: LayerNorm gives exactly 0
    x[6, 1000] = float("inf")                       # the mean is inf: every element of the row is NaN
    x = _strided_in_nan_parent(x)
    zero = torch.zeros(dim, dtype=BF, device="cuda")
    # a bf16 subnormal: the constant row's blocks hold only it, the scale clamps at code 0 = 2^-127 and every element is 1.0 (code 2)
    tiny_shift = torch.full((dim,), 2.0 ** -127, dtype=BF, device="cuda")
    for kw in (dict(scale1p=wide, shift=zero), dict(scale1p=wide), dict(scale1p=wide, shift=tiny_shift), dict()):
        got = ops.layernorm_modulate_mxfp4(x, **kw)
        _assert_same(got, _pair(ops, x, **kw), f"dim {dim} data classes {sorted(kw)}")
        c4, sc = got
        if "scale1p" in kw:
            live = sc[0].int()
            assert int(live.max()) - int(live.min()) >= 60, "the block scales of a row follow 1 + scale over 70 binades"
        if kw.get("shift") is tiny_shift:
            assert bool((sc[3] == 0).all()) and bool((c4[3] == 0x22).all()), "a block of bf16 subnormals: code 0, elements 1.0"
        else:
            assert bool((sc[3] == 127).all()) and bool((c4[3] == 0).all()), "a zero block: code 127, elements +0"
        assert bool((sc[6] == 255).all()) and bool((c4[6] == 0).all()), "a row with an inf: every block code 255 with zero elements"
        assert not bool((sc[[0, 1, 2, 4, 5, 7, 8]] == 255).any())


def test_layernorm_producer_falls_back_at_other_widths_with_the_same_bits(ops):
    g = torch.Generator().manual_seed(256)
    vec = _ln_vectors(256, g)
    x = _strided_in_nan_parent(torch.randn((9, 256), generator=g).to(BF))
    for names in OPSETS:
        kw = {n: vec[n] for n in names}
        _assert_same(ops.layernorm_modulate_mxfp4(x, **kw), _pair(ops, x, **kw), f"dim 256 operands {names}")


def _raw_ln(lib, x, out4, scales, vec, rows, dim, xs, os4, ss):
    rc = lib.gf_layernorm_modulate_mxfp4(_ptr(x), _ptr(out4), _ptr(scales), _ptr(vec.get("weight")), _ptr(vec.get("bias")), _ptr(vec.get("scale1p")),
                                         _ptr(vec.get("shift")), rows, dim, xs, os4, ss, 1e-6, _st())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("names", [("scale1p", "shift"), ("weight",)])
def test_layernorm_producer_writes_only_its_outputs_and_takes_no_rows(ops, lib, names):
    rows, dim = 9, 1536
    g = torch.Generator().manual_seed(99)
    vec = {n: v for n, v in _ln_vectors(dim, g).items() if n in names}
    x = _strided_in_nan_parent(torch.randn((rows, dim), generator=g).to(BF))
    (o4, p4), (os_, ps) = _ff_parent(rows, dim // 2, 16, 12), _ff_parent(rows, dim // 32, 5, 3)     # the scale rows at odd addresses
    assert _raw_ln(lib, x, o4, os_, vec, rows, dim, x.stride(0), o4.stride(0), os_.stride(0)) == 0, lib.gf_last_error()
    _assert_same((o4, os_), _pair(ops, x, **vec), f"strided outputs {names}")
    assert _only_the_view_was_written(p4, rows, 16, dim // 2) and _only_the_view_was_written(ps, rows, 5, dim // 32), "a store outside the outputs"
    p4.fill_(0xFF)
    ps.fill_(0xFF)
    assert _raw_ln(lib, x, o4, os_, vec, 0, dim, x.stride(0), o4.stride(0), os_.stride(0)) == 0
    assert bool((p4 == 0xFF).all()) and bool((ps == 0xFF).all()), "rows = 0 wrote something"


def test_layernorm_producer_refusals_by_message_with_outputs_untouched(lib):
    rows, dim = 5, 1536
    x = torch.zeros((rows, dim), dtype=BF, device="cuda")
    (o4, p4), (os_, ps) = _ff_parent(rows, 2048 // 2, 16, 16), _ff_parent(rows, 2048 // 32, 5, 3)
    vec = dict(scale1p=torch.ones(2048, dtype=BF, device="cuda"), shift=torch.zeros(2048, dtype=BF, device="cuda"))
    ok = dict(x=x, out4=o4, scales=os_, rows=rows, dim=dim, xs=dim, os4=o4.stride(0), ss=os_.stride(0))
    cases = [
        (dict(dim=2048, xs=2048), "dim=2048 is not one of the wave-per-row widths (5120, 4096, 1536); use gf_layernorm_modulate + gf_quant_mxfp4"),
        (dict(out4=o4.data_ptr() + 2), "4-byte (out4) aligned"),
        (dict(os4=dim // 2 - 4), "strides must be multiples of 8 (x) / 4 (out4) and cover the row"),
        (dict(os4=dim // 2 + 2), "strides must be multiples of 8 (x) / 4 (out4) and cover the row"),
        (dict(ss=dim // 32 - 1), "strides must be multiples of 8 (x) / 4 (out4) and cover the row"),
        (dict(x=None), "null x/out4/scales"), (dict(out4=None), "null x/out4/scales"), (dict(scales=None), "null x/out4/scales"),
        (dict(x=x.data_ptr() + 8), "16-byte (x)"),
    ]
    for change, msg in cases:
        a = dict(ok, **change)
        rc = _raw_ln(lib, a["x"], a["out4"], a["scales"], vec, a["rows"], a["dim"], a["xs"], a["os4"], a["ss"])
        err = lib.gf_last_error().decode()
        assert rc == GF_ERR_INVALID_ARG and err.startswith("gf_layernorm_modulate_mxfp4: ") and msg in err, (change, rc, err)
        assert bool((p4 == 0xFF).all()) and bool((ps == 0xFF).all()), f"{change}: a refused call wrote to its outputs"
    rc = lib.gf_layernorm_modulate_mxfp4(_ptr(x), _ptr(o4), _ptr(os_), None, None, vec["scale1p"].data_ptr() + 2, None, rows, dim, dim, o4.stride(0),
                                         os_.stride(0), 1e-6, _st())
    assert rc == GF_ERR_INVALID_ARG and "vectors must be 16-byte aligned" in lib.gf_last_error().decode()
    torch.cuda.synchronize()
    assert bool((p4 == 0xFF).all()) and bool((ps == 0xFF).all())


# ---------------------------------------------------------------------------------------------------------------------
# the GEMM producer: cases computed once and left unchanged
_CASES = {}


def _case(M, N, K):
    if (M, N, K) not in _CASES:
        d = F.gauss_inputs(M, N, K)
        _CASES[(M, N, K)] = {k: d[k].cuda() for k in ("a4", "sa", "w4", "sw", "bias")}
    return _CASES[(M, N, K)]


def _q4_pair(ops, v, epi, bias="bias", sa=None, sw=None):
    b = v[bias] if isinstance(bias, str) else bias
    sa, sw = v["sa"] if sa is None else sa, v["sw"] if sw is None else sw
    return ops.gemm_mxfp4_q4(v["a4"], sa, v["w4"], sw, b, epilogue=epi), ops.quant_mxfp4(ops.gemm_mxfp4(v["a4"], sa, v["w4"], sw, b, epilogue=epi))


@pytest.mark.parametrize("M,N,K", Q4_SHAPES)
def test_gemm_producer_equals_the_pair(ops, M, N, K):
    v = _case(M, N, K)
    for epi in Q4_EPIS:
        got, want = _q4_pair(ops, v, epi)
        assert tuple(got[0].shape) == (M, N // 2) and tuple(got[1].shape) == (M, N // 32) and got[0].dtype == got[1].dtype == U8
        _assert_same(got, want, f"q4 {M} x {N} x {K} {R.EPI_NAMES[epi]}")
        assert not bool((got[1] == 255).any()), "a NaN block: an operand or a scale was read outside its rows"
    got, want = _q4_pair(ops, v, R.EPI_GELU, bias=None)
    _assert_same(got, want, f"q4 {M} x {N} x {K} no bias")


def test_gemm_producer_on_wide_biases_zero_blocks_and_nan_scales(ops):
    M, N, K = 257, 288, 768
    v = _case(M, N, K)
    g = torch.Generator().manual_seed(5)
    # a bias whose 32-column blocks span 2^-20 .. 2^20: the blocks of one output row get scales 40 binades apart
    expo = torch.linspace(-20, 20, N // 32).round()
    wide = (torch.randn(N, generator=g) * torch.exp2(expo).repeat_interleave(32)).to(BF).cuda()
    for epi in Q4_EPIS:
        got, want = _q4_pair(ops, v, epi, bias=wide)
        _assert_same(got, want, f"wide bias {R.EPI_NAMES[epi]}")
    assert int(got[1][0].int().max()) - int(got[1][0].int().min()) >= 15
    # bias -11 under GELU: the outputs are -0 or tiny negatives (down to 1e-37), so whole blocks are zero blocks (code 127, elements +0)
    # and the rest have scales far below anything else here
    low = torch.full((N,), -11.0, dtype=BF, device="cuda")
    got, want = _q4_pair(ops, v, R.EPI_GELU, bias=low)
    _assert_same(got, want, "bias -11 under gelu")
    y = ops.gemm_mxfp4(v["a4"], v["sa"], v["w4"], v["sw"], low, epilogue=R.EPI_GELU)
    zero_block = (y.view(M, N // 32, 32) == 0).all(-1)
    assert bool(torch.signbit(y.float()).all()) and bool(zero_block.any()), "the class is meant to give -0 outputs and zero blocks"
    assert torch.equal(got[1] == 127, zero_block), "zero blocks, and only they, have code 127"
    assert bool((got[0].view(M, N // 32, 16)[zero_block] == 0).all()), "a zero block's elements are +0"
    # one NaN scale in a row of A and in a row of W: row 5 and column 9 are NaN, so row 5's blocks and every row's block 0 are code 255
    sa, sw = v["sa"].clone(), v["sw"].clone()
    sa[5, 3], sw[9, 20] = 255, 255
    for epi in Q4_EPIS:
        got, want = _q4_pair(ops, v, epi, sa=sa, sw=sw)
        _assert_same(got, want, f"NaN scales {R.EPI_NAMES[epi]}")
        c4, sc = got
        bad = torch.zeros_like(sc, dtype=torch.bool)
        bad[5] = True
        bad[:, 0] = True
        assert torch.equal(sc == 255, bad), "NaN blocks: row 5 and block 0 of every row, nothing else"
        assert bool((c4[5] == 0).all()) and bool((c4[:, :16] == 0).all()), "a NaN block has zero elements"


def _raw_q4(lib, v, C4, ldc4, cs, lcs, M, N, K, epi, **over):
    a = dict(A=v["a4"], lda=K // 2, sa=v["sa"], lsa=K // 32, W=v["w4"], ldw=K // 2, sw=v["sw"], lsw=K // 32, bias=v["bias"])
    a.update(over)
    rc = lib.gf_gemm_mxfp4_q4(_ptr(a["A"]), a["lda"], _ptr(a["sa"]), a["lsa"], _ptr(a["W"]), a["ldw"], _ptr(a["sw"]), a["lsw"], _ptr(a["bias"]),
                              _ptr(C4), ldc4, _ptr(cs), lcs, M, N, K, epi, _st())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("M,N,K", [(257, 288, 768), (17, 64, 256)])
def test_gemm_producer_writes_only_its_outputs_and_takes_no_rows(ops, lib, M, N, K):
    """ldc4 = N/2 + 16 and c_scale_stride = N/32 + 3 inside 0xFF parents that also hold rows past M."""
    v = _case(M, N, K)
    for epi in Q4_EPIS:
        (C4, p4), (cs, ps) = _ff_parent(M, N // 2, 0, 16), _ff_parent(M, N // 32, 0, 3)
        assert C4.stride(0) == N // 2 + 16 and cs.stride(0) == N // 32 + 3
        assert _raw_q4(lib, v, C4, C4.stride(0), cs, cs.stride(0), M, N, K, epi) == 0, lib.gf_last_error()
        _assert_same((C4, cs), ops.quant_mxfp4(ops.gemm_mxfp4(v["a4"], v["sa"], v["w4"], v["sw"], v["bias"], epilogue=epi)), f"strided C4 {M} x {N} x {K} {epi}")
        assert _only_the_view_was_written(p4, M, 0, N // 2) and _only_the_view_was_written(ps, M, 0, N // 32), "a store in a gap or past row M"
    p4.fill_(0xFF)
    ps.fill_(0xFF)
    assert _raw_q4(lib, v, C4, C4.stride(0), cs, cs.stride(0), 0, N, K, 0) == 0
    assert bool((p4 == 0xFF).all()) and bool((ps == 0xFF).all()), "M = 0 wrote something"
    e4, es = ops.gemm_mxfp4_q4(v["a4"][:0], v["sa"][:0], v["w4"], v["sw"])
    assert tuple(e4.shape) == (0, N // 2) and tuple(es.shape) == (0, N // 32)


def test_gemm_producer_feeds_the_next_gemm(ops):
    """(c4, c_scale) straight into gemm_mxfp4 equals the unfused chain: GEMM, quantiser, GEMM."""
    M, N, K, N2 = 129, 256, 256, 64
    v = _case(M, N, K)
    g = torch.Generator().manual_seed(3)
    w2 = ops.quant_mxfp4((torch.randn((N2, N), generator=g) / 16).to(BF).cuda())
    c4, cs = ops.gemm_mxfp4_q4(v["a4"], v["sa"], v["w4"], v["sw"], v["bias"], epilogue=R.EPI_GELU)
    u4, us = ops.quant_mxfp4(ops.gemm_mxfp4(v["a4"], v["sa"], v["w4"], v["sw"], v["bias"], epilogue=R.EPI_GELU))
    got, want = ops.gemm_mxfp4(c4, cs, w2[0], w2[1]), ops.gemm_mxfp4(u4, us, w2[0], w2[1])
    assert bool(torch.isfinite(got).all()) and torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_gemm_producer_refusals_by_message_with_outputs_untouched(ops, lib):
    M, N, K = 17, 64, 256
    v = _case(M, N, K)
    (C4, p4), (cs, ps) = _ff_parent(M, N // 2, 0, 16), _ff_parent(M, N // 32, 0, 3)
    ok = dict(C4=C4, ldc4=C4.stride(0), cs=cs, lcs=cs.stride(0), M=M, N=N, K=K, epi=0)
    cases = [
        (dict(N=40), "N=40 must be a multiple of 32"),
        (dict(epi=2), "epilogue 2 takes a second operand"), (dict(epi=3), "epilogue 3 takes a second operand"),
        (dict(epi=5), "epilogue 5 takes a second operand"), (dict(epi=6), "unknown epilogue 6"),
        (dict(ldc4=N // 2 + 8), "leading dimensions must be multiples of 16"), (dict(ldc4=N // 2 - 16), "leading dimensions must be multiples of 16"),
        (dict(lcs=N // 32 - 1), "c_scale_stride must cover N/32 = 2 blocks"),
        (dict(C4=C4.data_ptr() + 8), "16-byte alignment required"), (dict(A=v["a4"].data_ptr() + 8), "16-byte alignment required"),
        (dict(C4=None), "null A/W/C/scales"), (dict(cs=None), "null A/W/C/scales"), (dict(sa=None), "null A/W/C/scales"),
        (dict(K=K - 128), "K=128 must be a multiple of 256"), (dict(lda=K // 2 + 8), "leading dimensions must be multiples of 16"),
        (dict(lsa=K // 32 - 1), "scale strides must cover K/32 = 8 blocks"), (dict(M=1 << 30), "M/N too large"),
        (dict(lda=1 << 24), "operand too large for 32-bit staging offsets"),
    ]
    for change, msg in cases:
        a = dict(ok, **change)
        over = {k: a[k] for k in ("A", "lda", "sa", "lsa") if k in change}
        rc = _raw_q4(lib, v, a["C4"], a["ldc4"], a["cs"], a["lcs"], a["M"], a["N"], a["K"], a["epi"], **over)
        err = lib.gf_last_error().decode()
        assert rc == GF_ERR_INVALID_ARG and err.startswith("gf_gemm_mxfp4_q4: ") and msg in err, (change, rc, err)
        assert bool((p4 == 0xFF).all()) and bool((ps == 0xFF).all()), f"{change}: a refused call wrote to its outputs"
    # the wrapper's own words, before the library is called
    from goal_force_amd._lib import GoalForceError
    w40 = (v["w4"][:40], v["sw"][:40])
    with pytest.raises(GoalForceError, match="N = 40 output features must be a multiple of 32"):
        ops.gemm_mxfp4_q4(v["a4"], v["sa"], *w40)
    for epi in (2, 3, 5):
        with pytest.raises(GoalForceError, match=f"gemm_mxfp4_q4: epilogue {epi} is not one of"):
            ops.gemm_mxfp4_q4(v["a4"], v["sa"], v["w4"], v["sw"], v["bias"], epilogue=epi)
    for kw, msg in ((dict(a4=v["a4"].view(torch.int8)), "expected dtype torch.uint8"), (dict(a_scale=v["sa"][:, :-1]), "activation scales: expected"),
                    (dict(w_scale=None), "weight scales: required"), (dict(w4=v["w4"][:, :-16]), "weight: expected"),
                    (dict(bias=v["bias"][:-8]), "gemm_mxfp4_q4.bias: expected contiguous")):
        with pytest.raises(GoalForceError, match=msg):
            ops.gemm_mxfp4_q4(**dict(dict(a4=v["a4"], a_scale=v["sa"], w4=v["w4"], w_scale=v["sw"], bias=v["bias"]), **kw))


# ---------------------------------------------------------------------------------------------------------------------
# the module: the FFN of an enable_fp4 block in three launches
S, CTX, GRID = 300, 64, (3, 10, 10)


def _block_and_inputs(dim, heads, ffn):
    import sys
    from conftest import GOLDEN
    sys.path.insert(0, GOLDEN)
    import gen_inputs as gi
    from goal_force_amd.dit import DiTBlock, RopeTable, precompute_freqs_cis_3d
    sd = gi.block_sd(torch.Generator().manual_seed(61), dim, ffn, "", BF)
    x, ctx, t_mod = gi.block_inputs(dim, S, CTX, seed=62)
    blk = DiTBlock(False, dim, heads, ffn, 1e-6)
    blk.load_state_dict(sd, strict=True)
    rope = RopeTable.from_grid(precompute_freqs_cis_3d(dim // heads), *GRID, "cuda")
    return blk.to(BF).cuda(), (x.cuda(), ctx.cuda(), t_mod.cuda(), rope)


def _restated_linear(dit, real):
    """dit.linear with every enable_fp4 layer restated (test_fp4_gpu.py's): fp64 product of the fake-quantised input and weight, then the
    epilogue's chain — every other layer goes to the real function."""
    def linear(x2, lin, epilogue=0, resid=None, gate=None, out=None):
        if getattr(lin, "_gf_w4", None) is None:
            return real(x2, lin, epilogue=epilogue, resid=resid, gate=gate, out=out)
        assert x2.dtype == BF, "an enable_fp4 layer is handed bf16"
        linear.restated += 1
        acc = F.fake_quant(x2.cpu()) @ F.fake_quant(lin.weight.detach().cpu()).t()
        y = R.chain(acc, lin.bias.detach().cpu(), int(epilogue), None if resid is None else resid.cpu(), None if gate is None else gate.cpu())[0]
        y = y.to(BF).cuda()
        return y if out is None else out.copy_(y)
    linear.restated = 0
    return linear


def _count_quant_calls(monkeypatch, ops):
    calls, real = [], ops.quant_mxfp4

    def counted(x):
        calls.append(tuple(x.shape))
        return real(x)
    monkeypatch.setattr(ops, "quant_mxfp4", counted)
    return calls


@pytest.mark.parametrize("layers", [("ffn",), ("ffn", "o")])
@pytest.mark.parametrize("fp8", [False, True])
def test_block_fused_equals_unfused_and_the_restatement(monkeypatch, ops, layers, fp8):
    """dim 1536: the LayerNorm is the fused kernel.  Fused on: no stand-alone quantiser pass for the FFN (2 remain for the "o" layers);
    the same bits as with the option off; and with it off the block equals the fp64 restatement of its fp4 layers."""
    from goal_force_amd import dit
    blk, inputs = _block_and_inputs(1536, 12, 1024)
    if fp8:
        dit.enable_fp8(blk)
    before = blk(*inputs).clone()
    dit.enable_fp4(blk, layers=layers)
    calls = _count_quant_calls(monkeypatch, ops)
    assert ops.option("fp4_fused")
    fused = blk(*inputs).clone()
    assert len(calls) == (2 if "o" in layers else 0), f"stand-alone quantiser passes with the fused FFN: {calls}"
    del calls[:]
    with ops.options(fp4_fused=False):
        unfused = blk(*inputs).clone()
        assert len(calls) == (4 if "o" in layers else 2), calls
        monkeypatch.undo()
        restated = _restated_linear(dit, dit.linear)
        monkeypatch.setattr(dit, "linear", restated)
        ref = blk(*inputs).clone()
        monkeypatch.undo()
        assert restated.restated == (4 if "o" in layers else 2), "the restatement did not see every fp4 layer"
    assert bool(torch.isfinite(fused).all()) and not torch.equal(fused, before)
    assert torch.equal(fused.view(torch.int16), unfused.view(torch.int16)), "the fused FFN changes the block's bits"
    e = float((unfused.float() - ref.float()).norm() / ref.float().norm())
    print(f"PIN enable_fp4 block dim 1536 layers={layers} fp8={fp8}: rel-L2 of the unfused block to the restated block {e:.3e}")
    assert e < 5e-3, f"rel-L2 {e:.3e}"
    dit.enable_fp4(blk, False)
    assert torch.equal(blk(*inputs), before)


@pytest.mark.parametrize("fp8", [False, True])
def test_block_at_the_fallback_width(ops, fp8):
    """dim 256: the LayerNorm producer falls back to its pair, the GELU GEMM's epilogue is still the fused one."""
    from goal_force_amd import dit
    blk, inputs = _block_and_inputs(256, 2, 512)
    if fp8:
        dit.enable_fp8(blk)
    dit.enable_fp4(blk)
    fused = blk(*inputs).clone()
    with ops.options(fp4_fused=False):
        unfused = blk(*inputs).clone()
    assert bool(torch.isfinite(fused).all()) and torch.equal(fused.view(torch.int16), unfused.view(torch.int16))


def test_a_changed_master_refreshes_the_copies_on_the_fused_route(ops):
    from goal_force_amd import dit
    blk, inputs = _block_and_inputs(256, 2, 512)
    dit.enable_fp4(blk, layers=("ffn",))
    first = blk(*inputs).clone()
    blk.ffn[0].weight.mul_(0.5)
    blk.ffn[2].weight.mul_(2.0)
    fused = blk(*inputs).clone()
    with ops.options(fp4_fused=False):
        unfused = blk(*inputs).clone()
    assert not torch.equal(fused, first) and torch.equal(fused.view(torch.int16), unfused.view(torch.int16))


def test_pipeline_fused_equals_unfused_and_off_restores_the_base(ops):
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
    fused = forward()
    with ops.options(fp4_fused=False):
        unfused = forward()
    assert bool(torch.isfinite(fused).all()) and not torch.equal(fused, base)
    assert torch.equal(fused.view(torch.int16), unfused.view(torch.int16)), "the fused FFN changes the model's bits"
    dit.enable_fp4(pipe, False)
    assert torch.equal(forward(), base)
