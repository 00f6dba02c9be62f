"""The forward row and elementwise kernels (gf_rowops.hip, gf_elementwise.hip) pinned element by element, at every dispatch path.

LayerNorm, RMSNorm(+RoPE) and rope_apply are held against the exact chains of tests/forward_refs.py (fp64 arithmetic, bf16 roundings
where the reference has them) through two bars, no element left out:  (a) the bf16 bits differ on at most 2^-10 of the elements,
(b) every element is within 2^-7 m + 2^-16 s.  tests/test_forward_refs_cpu.py shows on the CPU, on the SAME inputs (the case lists are
shared), that an fp32 restatement of each chain passes both and that a dropped intermediate rounding, `scale` for `1 + scale`, a RoPE pair
index without `% head_dim`, a mean over all but the last 8 columns and a flipped sign of sin do not.  The operations that are plain bf16
eager arithmetic get no tolerance: torch.equal against torch's CPU result or oracle.fp8_oracle.  gf_act and gf_cast_fp8 have a 16-bit
input and are run on all 65 536 bit patterns.

Which case reaches which kernel:
  layernorm_modulate_kernel (128 threads per row)         widths 8 / 264 / 2048 / 8192 of test_layernorm_every_path
  layernorm_wave2_kernel<NCH, MODE, false>                widths 1536 / 4096 / 5120 with the sets plain, weight+bias, scale1p+shift
  layernorm_modulate_wave_kernel<NCH, LN_BF16>            width 5120 with the 13 other operand sets (the partial sets; the general
                                                          kernel gets all 16 at width 264)
  layernorm_modulate_wave_kernel<NCH, LN_FP8>             test_layernorm_fp8_partial_operand_sets (every set but the three above)
  layernorm_wave2_kernel<NCH, MODE, true>                 the same test's three DiT sets
  rmsnorm_rope_kernel                                     widths 8 / 264 / 2048 / 8192 of test_rmsnorm_rope_every_path
  rmsnorm_rope_wave_kernel<NCH, 0 | 1>                    widths 1536 / 4096 / 5120 without a table | head_dim 128, 64, 8
  rmsnorm_rope_wave_kernel<NCH, ROPE = 2>                 forward_refs.ROPE2_SHAPES: 1536 with head_dim 96, 768; 5120 with 40, 320, 1024,
                                                          5120; 4096 with 1024, 4096 (test_the_rope2_cases_are_there keeps them listed)
  the grid-stride loops (grid capped at 2048 x 256)       rope_apply / modulate 1100 x 3840 (528 000 chunks), gate_residual 1100 x 4096,
                                                          add / sub / cfg_euler n = 4 200 453 (tail of 5), act n = 525 291,
                                                          modulation 32 x 16392, patchify 599 040 slots, unpatchify 549 120 pairs
  modulation_kernel                                       test_modulation
Every pinned case prints a line `PIN` with its differing share and its worst share of the allowance (`pytest -s`).
"""
import pytest
import torch

import forward_refs as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FP8 = torch.float8_e4m3fn
SENTINEL = 0x5A5A           # a finite bf16 bit pattern no kernel here produces by accident in a whole margin
BIG_N = 2048 * 256 * 8 + 6149       # past the grid cap of the 16-byte elementwise kernels, n % 8 = 5


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from goal_force_amd import ops as _ops
    return _ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _c(t):
    return None if t is None else t.cuda()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _sub_id(sub):
    return "+".join(sub) or "plain"


def _ln_id(c):
    return f"{c[0]}x{c[1]}-{_sub_id(c[2])}"


def _rms_id(c):
    return f"{c[0]}x{c[1]}-hd{c[2]}-t{c[3]}"


def _guarded(t):
    """t [rows, dim] bf16 placed as a column slice of a wider sentinel-filled GPU buffer with margins left, right and below ->
    (buffer, view)."""
    rows, dim = t.shape
    buf = torch.full((rows + 3, dim + 40), SENTINEL, dtype=torch.int16, device="cuda").view(BF)
    view = buf[:rows, 16:16 + dim]
    view.copy_(t.cuda())
    return buf, view


def _margins_untouched(buf, view, what):
    rows, dim = view.shape
    torch.cuda.synchronize()
    margins = buf.view(torch.int16).clone()
    margins[:rows, 16:16 + dim] = SENTINEL
    assert bool((margins == SENTINEL).all()), f"{what}: wrote outside its rows ({int((margins != SENTINEL).sum())} elements)"


# ---------------------------------------------------------------------------------------------------------------------
# F1 gf_layernorm_modulate
@pytest.mark.parametrize("case", R.ln_cases(), ids=_ln_id)
def test_layernorm_every_path(ops, case):
    """13 rows: x and out are column slices of wider buffers (two different strides, the guard columns must stay), with a constant row,
    an all-zero row, a row of 300 + noise and a row scaled by 1e3; 1 row: contiguous.  Then out aliasing x: the same bits.
    The 300 + noise row is drawn clear of the bf16 rounding boundaries (forward_refs.offset_row), so by construction it cannot trip
    (a): it tests the cancellation in x - mean through (b) and the magnitude of the result, not (a)."""
    rows, dim, sub = case
    x, v = R.ln_inputs(rows, dim, sub)
    chain, m = R.layernorm_chain(x, **v)
    kw = {k: _c(t) for k, t in v.items()}
    what = f"layernorm {_ln_id(case)}"
    if rows == 1:
        xg = x.cuda()
        got = ops.layernorm_modulate(xg, **kw)
    else:
        xw = torch.zeros((rows, dim + 24), dtype=BF, device="cuda")
        xg = xw[:, 8:8 + dim]
        xg.copy_(x.cuda())
        buf, got = _guarded(torch.zeros_like(x))
        assert xg.stride(0) != got.stride(0) and not xg.is_contiguous()
        ops.layernorm_modulate(xg, out=got, **kw)
        _margins_untouched(buf, got, what)
    assert got.dtype == BF and got.shape == x.shape
    R.assert_pinned(got.cpu(), chain, m, what)
    alias = xg.clone()
    ops.layernorm_modulate(alias, out=alias, **kw)
    assert torch.equal(_bits(alias), _bits(got)), f"{what}: out aliasing x gives other bits"


def test_layernorm_refuses_widths_outside_its_range(ops):
    from goal_force_amd._lib import GoalForceError
    for dim in (8200, 12):
        x = torch.zeros((4, dim), dtype=BF, device="cuda")
        with pytest.raises(GoalForceError, match="multiple of 8 and <= 8192"):
            ops.layernorm_modulate(x)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# F2 gf_layernorm_modulate_fp8
@pytest.mark.parametrize("dim", [5120, 4096, 1536])
def test_layernorm_fp8_partial_operand_sets(ops, dim):
    """Every operand set at 5120, the four-operand set, the four single operands and the DiT sets at 4096 / 1536: e4m3 codes and scales
    bit-identical to gf_layernorm_modulate + gf_quant_fp8_rowscale, and that pair bit-identical to the oracle's quantize_activation.
    Column 3 of every vector is large, so every row with a non-zero normalisation has a maximum above 448 (scale_a > 1); the all-zero
    and the constant row have y = 0 and, without bias or shift, an all-zero result (scale_a = 1, codes +-0)."""
    from oracle import fp8_oracle
    subsets = R.SUBSETS if dim == 5120 else [s for s in R.SUBSETS if len(s) in (1, 4) or s in R.DIT_SETS]
    for sub in subsets:
        x, v = R.ln_inputs(13, dim, sub)
        for name, big in (("weight", 400.0), ("bias", 500.0), ("scale1p", 400.0), ("shift", 600.0)):
            if v[name] is not None:
                v[name][3] = big
        kw = {k: _c(t) for k, t in v.items()}
        xg = x.cuda()
        ln = ops.layernorm_modulate(xg, **kw)
        want8, wants = ops.quant_fp8_rowscale(ln)
        got8, gots = ops.layernorm_modulate_fp8(xg, **kw)
        what = f"layernorm_fp8 13x{dim} {_sub_id(sub)}"
        assert torch.equal(gots, wants), f"{what}: scales differ"
        assert torch.equal(got8.view(torch.uint8), want8.view(torch.uint8)), f"{what}: codes differ"
        ref8, refs = fp8_oracle.quantize_activation(ln.cpu())
        assert torch.equal(gots.cpu(), refs.reshape(-1)) and torch.equal(got8.cpu().view(torch.uint8), ref8.view(torch.uint8)), what
        if sub:
            assert float(gots.max()) > 1.0, f"{what}: the case must exercise scale_a > 1"
        if not ({"bias", "shift"} & set(sub)):
            zero = R.SPECIAL_ROWS["zero"]
            assert float(gots[zero]) == 1.0 and not bool((got8[zero].view(torch.uint8) & 0x7F).any()), f"{what}: the all-zero row"


# ---------------------------------------------------------------------------------------------------------------------
# F3 gf_rmsnorm_rope
def test_the_rope2_cases_are_there():
    """The cases of rmsnorm_rope_wave_kernel<NCH, ROPE = 2>: a head_dim that does not divide 512 at the three wave widths."""
    assert R.ROPE2_SHAPES == [(1536, 96), (1536, 768), (5120, 40), (5120, 320), (5120, 1024), (5120, 5120), (4096, 1024), (4096, 4096)]
    assert all(512 % h and d % h == 0 and h % 8 == 0 for d, h in R.ROPE2_SHAPES)


@pytest.mark.parametrize("case", R.rms_cases(), ids=_rms_id)
def test_rmsnorm_rope_every_path(ops, case):
    """In place.  13 rows: x is a column slice of a wider buffer whose guard columns must stay, with an all-zero row (rstd = 1/sqrt(eps))
    and a row scaled by 1e3; unit-modulus and scaled (q pre-scale) tables."""
    rows, dim, hd, scale = case
    x, w, cos, sin = R.rms_inputs(rows, dim, hd, scale)
    chain, m = R.rmsnorm_rope_chain(x, w, cos, sin, hd or 8)
    what = f"rmsnorm_rope {_rms_id(case)}"
    if rows == 1:
        buf, xg = None, x.cuda()
    else:
        buf, xg = _guarded(x)
    ret = ops.rmsnorm_rope(xg, w.cuda(), _c(cos), _c(sin), head_dim=hd or 8, eps=1e-6)
    assert ret is xg
    if buf is not None:
        _margins_untouched(buf, xg, what)
    R.assert_pinned(xg.cpu(), chain, m, what)


# ---------------------------------------------------------------------------------------------------------------------
# F4 gf_rope_apply, gf_modulate, gf_gate_residual
ROPE_CASES = [c for c in R.rms_cases() if c[2] is not None and c[0] == 13] + [(r, d, h, 1.0) for r, d, h in R.BIG_ROPE]


@pytest.mark.parametrize("case", ROPE_CASES, ids=_rms_id)
def test_rope_apply(ops, case):
    """The widths and head_dim values of gf_rmsnorm_rope on a strided x, and 1100 x 3840 (528 000 chunks: the grid-stride loop
    iterates) with head_dim 96 and 128."""
    rows, dim, hd, scale = case
    x, _, cos, sin = R.rms_inputs(rows, dim, hd, scale)
    chain, m = R.rope_apply_chain(x, cos, sin, hd)
    buf, xg = _guarded(x)
    got = ops.rope_apply(xg, cos.cuda(), sin.cuda(), hd)
    assert got.is_contiguous() and got.shape == x.shape
    _margins_untouched(buf, xg, "rope_apply input")
    assert torch.equal(_bits(xg.cpu()), _bits(x)), "rope_apply must not write its input"
    R.assert_pinned(got.cpu(), chain, m, f"rope_apply {_rms_id(case)}")


WIDTHS = sorted({d for d, _ in R.RMS_SHAPES})


@pytest.mark.parametrize("rows,dim", [(r, d) for d in WIDTHS for r in R.ROWS] + [(1100, 3840)])
def test_modulate_is_torch_bf16_arithmetic(ops, rows, dim):
    g = _gen(rows + dim)
    x = R.row_x(rows, dim, g, "rms")
    scale, shift = (0.5 * torch.randn(dim, generator=g)).to(BF), (0.5 * torch.randn(dim, generator=g)).to(BF)
    _, xg = _guarded(x)
    got = ops.modulate(xg, shift.cuda(), scale.cuda())
    assert torch.equal(_bits(got.cpu()), _bits(x * (1 + scale) + shift))


@pytest.mark.parametrize("rows,dim", [(r, d) for d in WIDTHS for r in R.ROWS] + [(1100, 4096)])
def test_gate_residual_is_torch_bf16_arithmetic(ops, rows, dim):
    g = _gen(2 * rows + dim)
    x, r = R.row_x(rows, dim, g, "rms"), torch.randn((rows, dim), generator=g).to(BF)
    gate = torch.randn(dim, generator=g).to(BF)
    _, xg = _guarded(x)
    rw = torch.zeros((rows, dim + 8), dtype=BF, device="cuda")
    rg = rw[:, 8:]
    rg.copy_(r.cuda())
    got = ops.gate_residual(xg, gate.cuda(), rg)
    assert torch.equal(_bits(got.cpu()), _bits(x + gate * r))


# ---------------------------------------------------------------------------------------------------------------------
# F5 gf_modulation
@pytest.mark.parametrize("dim", [8, 13, 1536, 5120])
def test_modulation(ops, dim):
    """Row broadcast i % t_rows, every bit of onep_mask (bits at or above k select nothing), k up to 32."""
    for k, t_rows in ((6, 6), (6, 1), (2, 2), (32, 1), (32, 8)):
        g = _gen(100 * k + t_rows + dim)
        param, t = torch.randn((k, dim), generator=g).to(BF), torch.randn((t_rows, dim), generator=g).to(BF)
        for mask in (0, 0b010010, 0b10, 1 << 31, 0xFFFFFFFF):
            got = ops.modulation(param.cuda(), t.cuda(), mask)
            assert got.shape == (k, dim) and got.dtype == BF
            assert torch.equal(_bits(got.cpu()), _bits(R.modulation_ref(param, t, mask))), f"modulation k={k} t_rows={t_rows} mask={mask:#x}"


def test_modulation_past_the_grid_cap_and_refusals(ops):
    from goal_force_amd._lib import GoalForceError
    k, dim = 32, 16392                                                   # 524 544 elements > 2048 x 256
    g = _gen(3)
    param, t = torch.randn((k, dim), generator=g).to(BF), torch.randn((8, dim), generator=g).to(BF)
    got = ops.modulation(param.cuda(), t.cuda(), 0x80000001)
    assert torch.equal(_bits(got.cpu()), _bits(R.modulation_ref(param, t, 0x80000001)))
    z = lambda r: torch.zeros((r, 16), dtype=BF, device="cuda")         # noqa: E731
    with pytest.raises(GoalForceError, match="bad k=33"):
        ops.modulation(z(33), z(1), 0)
    with pytest.raises(GoalForceError, match="t_rows=7"):
        ops.modulation(z(6), z(7), 0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# F6 gf_add_bf16, gf_sub_bf16, gf_cfg_euler_step
@pytest.mark.parametrize("n", [5, 8, BIG_N])
def test_add_sub_cfg_euler_are_torch_bf16_arithmetic(ops, n):
    """n = 5: the tail alone; 8: one vector, no tail; 4 200 453: past the grid cap (the loop iterates) with a tail of 5."""
    assert BIG_N % 8 == 5 and BIG_N // 8 > 2048 * 256
    g = _gen(n)
    a, b, c = (torch.randn(n, generator=g).to(BF) for _ in range(3))
    ag, bg, cg = a.cuda(), b.cuda(), c.cuda()
    assert torch.equal(_bits(ops.add(ag, bg).cpu()), _bits(a + b))
    assert torch.equal(_bits(ops.sub(ag, bg).cpu()), _bits(a - b))
    t = ag.clone()
    assert ops.add(t, bg, out=t) is t and torch.equal(_bits(t.cpu()), _bits(a + b)), "add: out aliasing a"
    t = bg.clone()
    assert ops.sub(ag, t, out=t) is t and torch.equal(_bits(t.cpu()), _bits(a - b)), "sub: out aliasing b"
    for cfg, ds in ((5.0, -0.25), (4.3, -0.0371)):
        got = ops.cfg_euler_step(ag.clone(), bg, cg, cfg, ds)
        assert torch.equal(_bits(got.cpu()), _bits(R.cfg_euler_ref(a, b, c, cfg, ds))), f"cfg_euler n={n} cfg={cfg}"
        got = ops.cfg_euler_step(ag.clone(), bg, None, cfg, ds)
        assert torch.equal(_bits(got.cpu()), _bits(R.cfg_euler_ref(a, b, None, cfg, ds))), f"cfg_euler n={n} without nega"


# ---------------------------------------------------------------------------------------------------------------------
# F7 gf_act
@pytest.mark.parametrize("kind", ["silu", "gelu_tanh"])
def test_act_on_every_bf16_value(ops, kind):
    """All 65 536 bit patterns: finite inputs within one bf16 step of bf16(fp64 function), differing share <= 2^-10; +-0, +-inf and NaN
    in the class of torch's CPU result."""
    x = R.all_bf16()
    got = ops.act(x.cuda(), kind).cpu()
    R.assert_act(got, x, kind, f"act {kind}, all 65536 patterns")
    fn = torch.nn.functional.silu if kind == "silu" else (lambda t: torch.nn.functional.gelu(t, approximate="tanh"))
    special = ~torch.isfinite(x.float()) | (x.float() == 0)
    assert int(special.sum()) == 2 * 128 + 2
    assert torch.equal(R.value_class(got[special]), R.value_class(fn(x[special]))), f"act {kind}: a special input left its class"


@pytest.mark.parametrize("kind", ["silu", "gelu_tanh"])
def test_act_past_the_grid_cap(ops, kind):
    n = 524288 + 1003
    x = (3 * torch.randn(n, generator=_gen(n))).to(BF)
    R.assert_act(ops.act(x.cuda(), kind).cpu(), x, kind, f"act {kind} n={n}")


# ---------------------------------------------------------------------------------------------------------------------
# F8 gf_cast_fp8
def test_cast_fp8_on_every_bf16_value(ops):
    """All 65 536 bit patterns against torch's own `x.to(float8_e4m3fn)` on the CPU: the codes of every finite input bit-equal —
    |x| <= 464 rounds to nearest even (448 at most), |x| > 464 is NaN in torch — and a NaN or infinite input gives a NaN code."""
    x = R.all_bf16()
    got = ops.cast_fp8(x.cuda()).cpu().view(torch.uint8)
    want = x.to(FP8).view(torch.uint8)
    fin = torch.isfinite(x.float())
    diff = (got != want) & fin
    if bool(diff.any()):
        i = diff.nonzero().flatten()
        print(f"CAST {int(diff.sum())} finite inputs differ; first: x={x[i[0]].item()} got {int(got[i[0]]):#x} want {int(want[i[0]]):#x}; "
              f"|x| range {x[i].float().abs().min().item()} .. {x[i].float().abs().max().item()}")
    assert not bool(diff.any()), f"{int(diff.sum())} finite inputs cast to another code than torch's"
    assert bool(((got[~fin] & 0x7F) == 0x7F).all()), "a NaN or infinite input must give a NaN code"


# ---------------------------------------------------------------------------------------------------------------------
# F9 gf_quant_fp8_rowscale
@pytest.mark.parametrize("dim", [8, 520, 13824, 14336])
@pytest.mark.parametrize("rows", [1, 13])
def test_quant_fp8_rowscale_is_the_oracle(ops, rows, dim):
    """Row maxima 0, 448, 450, 452, 466, 1500, 3e4; x strided; through the C ABI, out8 a column slice whose guard bytes must stay."""
    from goal_force_amd import _lib
    from oracle import fp8_oracle
    x = R.quant_inputs(rows, dim, rows + dim)
    ref8, refs = fp8_oracle.quantize_activation(x)
    _, xg = _guarded(x)
    got8, gots = ops.quant_fp8_rowscale(xg)
    assert torch.equal(gots.cpu(), refs.reshape(-1)), "scales"
    assert torch.equal(got8.cpu().view(torch.uint8), ref8.view(torch.uint8)), "codes"
    buf = torch.full((rows + 2, dim + 32), 0xA5, dtype=torch.uint8, device="cuda")
    out8, scale = buf[:rows, 16:16 + dim], torch.empty(rows, dtype=torch.float32, device="cuda")
    rc = _lib.load().gf_quant_fp8_rowscale(xg.data_ptr(), out8.data_ptr(), scale.data_ptr(), rows, dim, xg.stride(0), out8.stride(0),
                                           torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(out8.cpu(), ref8.view(torch.uint8)) and torch.equal(scale.cpu(), refs.reshape(-1))
    guard = buf.clone()
    guard[:rows, 16:16 + dim] = 0xA5
    assert bool((guard == 0xA5).all()), "gf_quant_fp8_rowscale wrote outside out8"


def test_quant_fp8_rowscale_refuses_14344(ops):
    from goal_force_amd._lib import GoalForceError
    with pytest.raises(GoalForceError, match="<= 14336"):
        ops.quant_fp8_rowscale(torch.zeros((2, 14344), dtype=BF, device="cuda"))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# F10 gf_patchify_im2col, gf_unpatchify
def test_patchify_and_unpatchify_past_the_grid_cap(ops):
    """599 040 patch slots and 549 120 output pairs (> 2048 x 256): the reshape / permute of test_patchify_unpatchify_exact."""
    from oracle import wan_oracle as wo
    g = _gen(10)
    c0, c1, F, H, W, kpad = 16, 20, 8, 60, 104, 192
    assert F * (H // 2) * (W // 2) * (kpad // 4) > 2048 * 256
    lat, y = torch.randn((c0, F, H, W), generator=g).to(BF), torch.randn((c1, F, H, W), generator=g).to(BF)
    cols = ops.patchify_im2col(lat.cuda(), y.cuda(), kpad=kpad).cpu()
    c = c0 + c1
    ref = torch.cat([lat, y], 0).reshape(c, F, H // 2, 2, W // 2, 2).permute(1, 2, 4, 0, 3, 5).reshape(F * (H // 2) * (W // 2), 4 * c)
    assert cols.shape == (ref.shape[0], kpad) and torch.equal(_bits(cols[:, :4 * c]), _bits(ref))
    assert not bool(_bits(cols[:, 4 * c:]).any()), "the K padding columns must be zero"
    c, f, h, w = 16, 11, 30, 52
    assert c * f * 2 * h * w > 2048 * 256
    tok = torch.randn((f * h * w, 4 * c), generator=g).to(BF)
    assert torch.equal(_bits(ops.unpatchify(tok.cuda(), c, f, h, w).cpu()), _bits(wo.unpatchify(tok[None], (f, h, w), c)[0]))
