"""gf_gemm_fp8_lora through the raw C ABI and ops.gemm_fp8_lora, and adapters beside fp8 Linears on modules (lora.set_beside_fp8).

Kernel: torch.equal with the two-launch pair gf_gemm_fp8(GF_EPI_BIAS) + gf_lora_up on every shape of fp8_lora_refs.CASES, all six
epilogues, on the exact class (also torch.equal to the fp64 chain of the header's formula under the four elementary epilogues) and
on gauss operands from the project's quantisers; NaN-filled parents around every operand, sentinels around `out`.
Modules: a block under enable_fp8 with adapters on all ten Linears — strength 0 and detached are the plain fp8 block's bits and
launches, the fused route is asserted where it runs and equals the two-launch route bit for bit, every adapted layer equals its
composition from the pinned kernels, and the block is held to the fp64 statement of peft's forward on the block's weights by the plain
fp8 block's own distance from the fp64 plain forward."""
import pytest
import torch

import fp8_lora_refs as FL
import gemm_refs as G

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENT = 0x5A5A
GF_ERR_INVALID_ARG = -1
HAS_R = (G.EPI_GATE_RESID, G.EPI_RESID, G.EPI_MUL)


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


@pytest.fixture
def beside():
    from goal_force_amd import lora
    old = lora.set_beside_fp8(True)
    yield lora
    lora.set_beside_fp8(old)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16)


def _held(x, ld, fill=float("nan"), rows_behind=3):
    """x [rows, cols] as a view of row pitch ld inside a parent whose every other element is `fill` (NaN: a read outside the operand
    poisons the result); 16 elements in front keep the base 16-byte aligned."""
    rows, cols = x.shape
    one = torch.tensor(fill, dtype=torch.float32).to(x.dtype) if x.dtype != G.E4M3 else None
    parent = torch.empty(16 + (rows + rows_behind) * ld, dtype=x.dtype, device="cuda")
    if one is None:
        parent.view(torch.uint8).fill_(0x7F)          # the e4m3 NaN code
    else:
        parent.fill_(fill)
    v = parent[16:16 + rows * ld].view(rows, ld)[:, :cols]
    v.copy_(x)
    return v


class Out:
    """out [M, N] with ldo = N + 8 inside a sentinel-filled parent."""

    def __init__(self, M, N, init=None):
        self.ld = N + 8
        self.parent = torch.full((16 + (M + 3) * self.ld,), SENT, dtype=torch.int16, device="cuda")
        self.v = self.parent[16:16 + M * self.ld].view(M, self.ld)[:, :N].view(BF)
        if init is not None:
            self.v.copy_(init)
        self.mask = torch.ones_like(self.parent, dtype=torch.bool)
        self.mask[16:16 + M * self.ld].view(M, self.ld)[:, :N] = False

    def guards_ok(self):
        return bool((self.parent[self.mask] == SENT).all())

    def untouched(self):
        return bool((self.parent == SENT).all())


def _dev(d):
    """The operands of an input dict on the device, every one inside a NaN-filled parent with a gap in its rows."""
    M, K = d["a8"].shape
    N, rp = d["up"].shape
    return dict(a8=_held(d["a8"].cuda(), K + 16), w8=_held(d["w8"].cuda(), K + 32), row_scale=d["row_scale"].float().cuda(),
                bias=d["bias"].cuda(), t=_held(d["t"].cuda(), rp + 8), up=_held(d["up"].cuda(), rp + 16),
                resid=_held(d["resid"].cuda(), N + 24), gate=d["gate"].cuda(), scale=d["scale"])


def _gauss(ops, M, N, K, rp, r, scale):
    g = torch.Generator(device="cuda").manual_seed(M * 31 + N * 7 + K)

    def rn(*shape, s=1.0):
        return (torch.randn(shape, generator=g, device="cuda") * s).to(BF)
    a8, rs = ops.quant_fp8_rowscale(rn(M, K, s=3.0))
    t, up = torch.zeros(M, rp, dtype=BF, device="cuda"), torch.zeros(N, rp, dtype=BF, device="cuda")
    t[:, :r], up[:, :r] = rn(M, r), rn(N, r, s=r ** -0.5)
    return dict(a8=_held(a8, K + 16), w8=_held(ops.cast_fp8(rn(N, K, s=K ** -0.5)), K + 32), row_scale=rs, bias=rn(N), t=_held(t, rp + 8),
                up=_held(up, rp + 16), resid=_held(rn(M, N), N + 24), gate=rn(N), scale=scale)


def _p(t):
    return None if t is None else t.data_ptr()


def _fused(lib, v, out, ldo, epi, bias=True, **over):
    M, K = v["a8"].shape
    N, rp = v["up"].shape
    a = dict(lda=v["a8"].stride(0), ldw=v["w8"].stride(0), ldt=v["t"].stride(0), ld_up=v["up"].stride(0), rp=rp, scale=v["scale"], M=M, N=N,
             K=K, epi=epi, resid=v["resid"] if epi in HAS_R else None, ldr=v["resid"].stride(0), gate=v["gate"] if epi == G.EPI_GATE_RESID else None,
             ldo=ldo, t=v["t"], up=v["up"])
    a.update(over)
    return lib.gf_gemm_fp8_lora(_p(v["a8"]), a["lda"], _p(v["w8"]), a["ldw"], _p(v["row_scale"]), _p(v["bias"]) if bias else None, _p(a["t"]),
                                a["ldt"], _p(a["up"]), a["ld_up"], a["rp"], a["scale"], out, a["ldo"], a["M"], a["N"], a["K"], a["epi"],
                                _p(a["resid"]), a["ldr"], _p(a["gate"]), _st())


def _pair(lib, v, epi, bias=True):
    """The two launches through the raw ABI: gf_gemm_fp8(GF_EPI_BIAS) into a temporary, gf_lora_up with the epilogue."""
    M, K = v["a8"].shape
    N, rp = v["up"].shape
    y0 = torch.empty(M, N, dtype=BF, device="cuda")
    out = torch.empty(M, N, dtype=BF, device="cuda")
    assert lib.gf_gemm_fp8(_p(v["a8"]), v["a8"].stride(0), _p(v["w8"]), v["w8"].stride(0), _p(v["row_scale"]), _p(v["bias"]) if bias else None,
                           _p(y0), N, M, N, K, G.EPI_BIAS, None, 0, None, _st()) == 0
    assert lib.gf_lora_up(_p(y0), N, _p(v["t"]), v["t"].stride(0), _p(v["up"]), v["up"].stride(0), _p(out), N, M, N, rp, v["scale"], epi,
                          _p(v["resid"]) if epi in HAS_R else None, v["resid"].stride(0), _p(v["gate"]) if epi == G.EPI_GATE_RESID else None,
                          _st()) == 0
    return out


def _run(lib, v, epi, bias=True):
    M, N = v["a8"].shape[0], v["up"].shape[0]
    out = Out(M, N)
    rc = _fused(lib, v, out.v.data_ptr(), out.ld, epi, bias=bias)
    assert rc == 0, lib.gf_last_error().decode()
    torch.cuda.synchronize()
    assert out.guards_ok(), "a write outside out [M, N]"
    return out.v.clone()


@pytest.mark.parametrize("M,N,K,rp,r,scale", FL.CASES)
def test_fused_equals_the_pair_and_the_chain(ops, lib, M, N, K, rp, r, scale):
    """At one (M, N, K): the two exact classes at this shape's (rank, scale) — equal to the pair under all six epilogues and to the fp64
    chain under the four elementary ones — and gauss operands at ALL four ranks x four scales x six epilogues against the pair."""
    assert lib.gf_gemm_fp8_lora_ok(M, N, K, rp) == 1
    for cls, make in FL.EXACT.items():
        d = make(M, N, K, rp, r, scale)
        v = _dev(d)
        for epi in G.EPIS:
            got, want = _run(lib, v, epi), _pair(lib, v, epi)
            assert torch.equal(_bits(got), _bits(want)), (cls, epi, int((_bits(got) != _bits(want)).sum()))
            if epi in FL.EXACT_EPIS:
                assert torch.equal(got.double().cpu(), FL.chain(d, epi)), (cls, epi)
    for rp_g, r_g in FL.RANKS:
        v = _gauss(ops, M, N, K, rp_g, r_g, 1.0)
        for sc in FL.SCALES:
            v["scale"] = sc
            for epi in G.EPIS:
                got, want = _run(lib, v, epi), _pair(lib, v, epi)
                assert torch.equal(_bits(got), _bits(want)), ("gauss", rp_g, r_g, sc, epi, int((_bits(got) != _bits(want)).sum()))
    # two calls give the same bits; no bias; out aliasing resid equals the out-of-place result
    v = _gauss(ops, M, N, K, rp, r, scale)
    assert torch.equal(_bits(_run(lib, v, G.EPI_GELU)), _bits(_run(lib, v, G.EPI_GELU)))
    assert torch.equal(_bits(_run(lib, v, G.EPI_BIAS, bias=False)), _bits(_pair(lib, v, G.EPI_BIAS, bias=False)))
    for epi in (G.EPI_GATE_RESID, G.EPI_RESID):
        want = _run(lib, v, epi)
        io = Out(M, N, init=v["resid"])
        assert _fused(lib, v, io.v.data_ptr(), io.ld, epi, resid=io.v, ldr=io.ld) == 0
        torch.cuda.synchronize()
        assert io.guards_ok() and torch.equal(_bits(io.v), _bits(want)), epi


@pytest.mark.parametrize("M,N,K", FL.SHAPES)
def test_stagger_and_group_apply_as_in_the_plain_kernel(ops, lib, M, N, K):
    """a4_stagger 0 .. 3 x a4_group_m 0 / 4 at EACH shape (K = 128: one K tile, where the rotation wraps to nothing)."""
    i = FL.SHAPES.index((M, N, K))
    (rp, r), scale = FL.EXACT_AT[i]
    v = _gauss(ops, M, N, K, rp, r, scale if scale else 0.7)
    for stagger in (0, 1, 2, 3):
        for group_m in (0, 4):
            with ops.options(a4_stagger=stagger, a4_group_m=group_m):
                for epi in (G.EPI_BIAS, G.EPI_GATE_RESID, G.EPI_GELU):
                    assert torch.equal(_bits(_run(lib, v, epi)), _bits(_pair(lib, v, epi))), (stagger, group_m, epi)


def test_refusals_leave_out_untouched(ops, lib):
    v = _dev(FL.integer_inputs(512, 136, 256, 32, 4, 0.7))
    out = Out(512, 136)
    bad = [(dict(M=511), "outside the fused kernel's shapes"), (dict(K=192), "K=192 must be a multiple of 128"), (dict(rp=0), "rank_pad=0 must be"),
           (dict(rp=48), "rank_pad=48 must be"), (dict(rp=96, ldt=96, ld_up=96), "outside the fused kernel's shapes"),
           (dict(rp=512), "rank_pad=512 must be"), (dict(scale=float("inf")), "scale must be finite"), (dict(scale=float("nan")), "scale must be finite"),
           (dict(ldt=36), "ldt / ld_up must be multiples of 8"), (dict(ld_up=24), "ldt / ld_up must be multiples of 8"),
           (dict(lda=264), "leading dimensions must be multiples"), (dict(ldo=128), "leading dimensions must be multiples"),
           (dict(epi=G.EPI_RESID, resid=None), "residual epilogue needs"), (dict(epi=G.EPI_GATE_RESID, gate=None), "gate epilogue needs"),
           (dict(epi=9), "unknown epilogue 9"), (dict(t=None), "null t/up")]
    for change, msg in bad:
        rc = _fused(lib, v, out.v.data_ptr(), change.pop("ldo", out.ld), change.pop("epi", G.EPI_BIAS), **change)
        assert rc == GF_ERR_INVALID_ARG and msg in lib.gf_last_error().decode(), (change, msg, rc, lib.gf_last_error().decode())
    with ops.options(prefer_8wave=1):
        assert _fused(lib, v, out.v.data_ptr(), out.ld, G.EPI_BIAS) == GF_ERR_INVALID_ARG and "prefer_8wave" in lib.gf_last_error().decode()
    torch.cuda.synchronize()
    assert out.untouched()


def test_ok_equals_its_restatement(ops, lib):
    for c in FL.OK_TABLE:
        assert lib.gf_gemm_fp8_lora_ok(*c) == FL.ok_py(*c), c
    with ops.options(prefer_8wave=1):
        assert not any(lib.gf_gemm_fp8_lora_ok(*c) for c in FL.OK_TABLE)


class Count:
    """Counting wrappers around the library's two entry points: which route ran."""

    def __init__(self, ops, monkeypatch):
        self.n = dict(fused=0, up=0)
        lib = ops._lib.load()

        class Proxy:
            def __getattr__(_, name):
                fn = getattr(lib, name)
                key = {"gf_gemm_fp8_lora": "fused", "gf_lora_up": "up"}.get(name)
                if key is None:
                    return fn

                def counted(*a):
                    self.n[key] += 1
                    return fn(*a)
                return counted
        monkeypatch.setattr(ops._lib, "load", lambda: Proxy())

    def take(self):
        out, self.n = self.n, dict(fused=0, up=0)
        return out


@pytest.mark.parametrize("M,rp,fused_opt", [(64, 32, True), (511, 64, True), (640, 128, True), (640, 256, True), (640, 64, False), (640, 64, True)])
def test_the_wrapper_takes_the_route_ok_names_and_both_give_the_same_bits(ops, lib, monkeypatch, M, rp, fused_opt):
    N, K, r, scale = 264, 256, rp - 3, -1.3
    v = _gauss(ops, M, N, K, rp, r, scale)
    want = {e: _pair(lib, v, e) for e in G.EPIS}
    cnt = Count(ops, monkeypatch)
    fused = fused_opt and FL.ok_py(M, N, K, rp)
    with ops.options(fp8_lora_fused=fused_opt):
        for e in G.EPIS:
            got = ops.gemm_fp8_lora(v["a8"], v["row_scale"], v["w8"], v["bias"], v["t"], v["up"], scale, epilogue=e,
                                    resid=v["resid"] if e in HAS_R else None, gate=v["gate"] if e == G.EPI_GATE_RESID else None)
            assert cnt.take() == (dict(fused=1, up=0) if fused else dict(fused=0, up=1)), (e, fused)
            assert torch.equal(_bits(got), _bits(want[e])), e
        x = v["resid"].contiguous().clone()
        ops.gemm_fp8_lora(v["a8"], v["row_scale"], v["w8"], v["bias"], v["t"], v["up"], scale, epilogue=G.EPI_RESID, resid=x, out=x)
        assert torch.equal(_bits(x), _bits(want[G.EPI_RESID]))


# ---------------------------------------------------------------------------------------------------------------------
# modules
LAYERS = tuple(f"{a}.{p}" for a in ("self_attn", "cross_attn") for p in "qkvo") + ("ffn.0", "ffn.2")
SHAPES = {256: (256, 2, 1024), 512: (512, 4, 2048)}
GRIDS = {72: (2, 6, 6), 130: (2, 5, 13), 520: (1, 20, 26)}
CTX = 48
_MOD = {}


def _adapter_sd(sd, layers, rank, seed):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in layers:
        n, k = sd[name + ".weight"].shape
        out[f"{name}.lora_B.weight"] = (torch.randn((n, rank), generator=g) / k ** 0.5).to(BF)
        out[f"{name}.lora_A.weight"] = (torch.randn((rank, k), generator=g) / rank ** 0.5).to(BF)
    return out


def _setup(tokens, dim=256):
    SHAPE = SHAPES[dim]
    key = (tokens, dim)
    if key not in _MOD:
        import gen_inputs as gi
        from goal_force_amd.dit import RopeTable, precompute_freqs_cis_3d
        from oracle import wan_oracle as wo
        dim, heads, ffn = SHAPE
        sd = gi.block_sd(torch.Generator().manual_seed(281), dim, ffn, "", BF)
        x, ctx, t_mod = gi.block_inputs(dim, tokens, CTX, seed=282)
        ctx[0, 40:] = ctx[0, 40]
        rope = RopeTable.from_grid(precompute_freqs_cis_3d(128), *GRIDS[tokens], "cuda")
        _MOD[key] = dict(shape=SHAPE, sd=sd, sd_dev={k: v.cuda() for k, v in sd.items()}, dev=(x.cuda(), ctx.cuda(), t_mod.cuda(), rope),
                            cpu=(x, ctx, t_mod, wo.rope_freqs_3d(128, *GRIDS[tokens])))
    return _MOD[key]


def _block(s, fp8=True):
    from goal_force_amd import dit
    dim, heads, ffn = s["shape"]
    with torch.device("cuda"):
        blk = dit.DiTBlock(False, dim, heads, ffn, 1e-6)
    blk = blk.to(BF)
    blk.load_state_dict(s["sd_dev"], strict=True)
    return dit.enable_fp8(blk) if fp8 else blk


def _oracle(s, sd64):
    from oracle import wan_oracle as wo
    x, ctx, t_mod, freqs = s["cpu"]
    return wo.dit_block(x.double(), ctx.double(), t_mod.double(), freqs, sd64, "", s["shape"][1])


def _rel(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm())


def _launches(ops, fn):
    ops.PROFILE_GEMM = []
    try:
        out = fn().clone()
        return out, [p[2:] for p in ops.PROFILE_GEMM]
    finally:
        ops.PROFILE_GEMM = None


def _trace_linears(monkeypatch, dit, fn):
    """Run fn() with dit.linear recording every call: its input, layer, epilogue, the residual as it was BEFORE the call (the block
    updates it in place), the gate and a copy of the result."""
    calls, real = [], dit.linear

    def traced(x2, lin, epilogue=0, resid=None, gate=None, out=None):
        r0 = None if resid is None else resid.clone()
        y = real(x2, lin, epilogue=epilogue, resid=resid, gate=gate, out=out)
        calls.append(dict(x=x2, lin=lin, epi=epilogue, resid=r0, gate=gate, y=y.clone()))
        return y
    monkeypatch.setattr(dit, "linear", traced)
    try:
        return fn().clone(), calls
    finally:
        monkeypatch.setattr(dit, "linear", real)


@pytest.mark.parametrize("tokens,dim", [(72, 256), (130, 256), (520, 256), (130, 512), (520, 512)])
def test_block_under_enable_fp8_with_adapters_on_every_linear(ops, beside, monkeypatch, tokens, dim):
    import lora_refs as LR
    lora = beside
    s = _setup(tokens, dim)
    lsd = _adapter_sd(s["sd"], LAYERS, 16, 283)
    blk = _block(s)
    plain, l_plain = _launches(ops, lambda: blk(*s["dev"]))
    assert lora.attach(blk, lsd, alpha=0.0) == len(LAYERS)
    zero, l_zero = _launches(ops, lambda: blk(*s["dev"]))
    assert torch.equal(zero, plain) and l_zero == l_plain, "strength 0: the plain fp8 block's bits and launch list"
    lora.set_strength(blk, 0.7)
    cnt = Count(ops, monkeypatch)
    att = blk(*s["dev"]).clone()
    n = cnt.take()
    # the self-attention's and the FFN's layers see all tokens; the cross-attention's k / v see the 41 folded context rows
    assert n == (dict(fused=8, up=2) if tokens >= 512 else dict(fused=0, up=10)), n
    assert not torch.equal(att, plain) and bool(torch.isfinite(att).all())
    with ops.options(fp8_lora_fused=False):
        assert torch.equal(blk(*s["dev"]), att), "fp8_lora_fused on = off"
        assert cnt.take() == dict(fused=0, up=10)
    monkeypatch.undo()
    # every one of the ten adapted layers, at the input the block gave it, is its composition from the kernels pinned above — with
    # the adapter's bf16 input derived HERE (the LayerNorms recomputed from the traced residual stream), not taken from the handle
    from goal_force_amd import dit
    traced, calls = _trace_linears(monkeypatch, dit, lambda: blk(*s["dev"]))
    assert torch.equal(traced, att) and len(calls) == 10
    x2 = s["dev"][0][0]
    sa, ca = blk.self_attn, blk.cross_attn
    by = {id(c["lin"]): c for c in calls}
    mod = ops.modulation(blk.modulation, s["dev"][2].contiguous(), onep_mask=0b010010)
    src = {id(m): ops.layernorm_modulate(x2, eps=blk.eps, scale1p=mod[1], shift=mod[0]) for m in (sa.q, sa.k, sa.v)}
    src[id(ca.q)] = ops.layernorm_modulate(by[id(sa.o)]["y"], eps=blk.eps, weight=blk.norm3.weight, bias=blk.norm3.bias)
    src[id(blk.ffn[0])] = ops.layernorm_modulate(by[id(ca.o)]["y"], eps=blk.eps, scale1p=mod[4], shift=mod[3])
    for c in calls:
        lin = c["lin"]
        (ad,) = lora.adapters(lin)
        given = c["x"]
        if id(lin) in src:
            assert isinstance(given, dit.QuantizedInput) and torch.equal(given.x2, src[id(lin)]), "the handle's source is the LayerNorm's bf16 row"
            xb = src[id(lin)]
        else:
            xb = given.x2 if isinstance(given, dit.QuantizedInput) else given
        a8, sc = ops.quant_fp8_rowscale(xb)
        if isinstance(given, dit.QuantizedInput):
            assert torch.equal(given.data.view(torch.uint8), a8.view(torch.uint8)) and torch.equal(given.scale, sc)
        want = ops.lora_up(ops.gemm_fp8(a8, sc, dit.fp8_weight(lin), lin.bias), ops.gemm(xb, ad.down), ad.up, 0.7, epilogue=c["epi"],
                           resid=c["resid"], gate=c["gate"])
        assert torch.equal(want, c["y"]), [n for n, m in blk.named_modules() if m is lin]
    # two adapters on one layer: their sequential application
    lsd2 = _adapter_sd(s["sd"], ("ffn.0",), 33, 284)
    lora.attach(blk, lsd2, alpha=-0.5, name="b")
    lin = blk.ffn[0]
    a, b = lora.adapters(lin)
    a8, sc = ops.quant_fp8_rowscale(x2)
    y = ops.lora_up(ops.gemm_fp8(a8, sc, dit.fp8_weight(lin), lin.bias), ops.gemm(x2, a.down), a.up, 0.7)
    y = ops.lora_up(y, ops.gemm(x2, b.down), b.up, -0.5, epilogue=ops.EPI_BIAS_GELU_TANH)
    assert torch.equal(dit.linear(x2, lin, epilogue=ops.EPI_BIAS_GELU_TANH), y)
    lora.detach(blk, "b")
    assert torch.equal(blk(*s["dev"]), att)
    # the fp64 statement: peft's unmerged forward is the block on W + s B A; the fp8 block's own distance from fp64 is the yardstick
    sd64 = {k: v.double() for k, v in s["sd"].items()}
    sd_peft = dict(sd64)
    for name in LAYERS:
        sd_peft[name + ".weight"] = sd64[name + ".weight"] + LR.f32(0.7) * (lsd[name + ".lora_B.weight"].double() @ lsd[name + ".lora_A.weight"].double())
    e_att, e_plain = _rel(att, _oracle(s, sd_peft)), _rel(plain, _oracle(s, sd64))
    print(f"PIN fp8 block with ten adapters, {tokens} tokens: rel-L2 from fp64 peft {e_att:.3e}; plain fp8 block from fp64 {e_plain:.3e}")
    assert e_att <= 1.25 * e_plain, (e_att, e_plain)
    assert lora.detach(blk) == len(LAYERS)
    off, l_off = _launches(ops, lambda: blk(*s["dev"]))
    assert torch.equal(off, plain) and l_off == l_plain, "detached: the plain fp8 block's bits and launch list"


def test_the_switch_off_keeps_the_refusals_on_the_device(ops):
    from goal_force_amd import lora
    from goal_force_amd._lib import GoalForceError
    assert lora.beside_fp8() is False
    s = _setup(72)
    blk = _block(s)
    with pytest.raises(GoalForceError, match=r"lora\.attach: 'self_attn\.q' carries an enable_fp8 weight copy"):
        lora.attach(blk, _adapter_sd(s["sd"], LAYERS, 4, 285))


def test_pipeline_call_under_enable_fp8_with_an_attached_adapter(beside):
    import gen_inputs as gi
    from goal_force_amd import dit
    from goal_force_amd.dit import WanModel
    from goal_force_amd.pipeline import WanVideoPipeline
    lora = beside
    cfg = gi.TINY
    dsd = gi.dit_sd(cfg, seed=41)
    m = WanModel(has_image_input=False, require_clip_embedding=False, **cfg)
    m.load_state_dict(dsd, strict=True)
    pipe = WanVideoPipeline.from_modules(dit.enable_fp8(m.to(BF).cuda()))
    dev = {k: v.cuda() for k, v in gi.tiny_inputs().items()}

    def run():
        return pipe.denoise(dev["latents"], dev["ctx_posi"], dev["ctx_nega"], dev["y"], None, num_inference_steps=2, cfg_scale=5.0,
                            controlnet=False).clone()
    plain = run()
    names = [f"blocks.{b}.{l}" for b in range(cfg["num_layers"]) for l in LAYERS]
    assert lora.attach(pipe.dit, _adapter_sd(dsd, names, 8, 286), alpha=0.7) == len(names)
    att = run()
    assert bool(torch.isfinite(att).all()) and not torch.equal(att, plain)
    assert torch.equal(run(), att)
    assert lora.detach(pipe.dit) == len(names)
    assert torch.equal(run(), plain)


# ---------------------------------------------------------------------------------------------------------------------
# the tape: trainable adapters beside a frozen fp8 block (references, restatement and bars: fp8_lora_refs' tape section)
TAPE_CASES = {c["name"]: c for c in FL.tape_cases()}
TARGETS = "q,k,v,o,ffn.0,ffn.2"
_TAPE = {}


def _tape_case(name):
    """(inputs, adapters, fp64 reference, restatement of order 0) — computed once on the host and left unchanged."""
    if name not in _TAPE:
        import gen_inputs as gi
        import lora_train_refs as LT
        import tape_refs as TP
        case = TAPE_CASES[name]
        cfg, sd, x, ctx, t_mod, dout = TP.case_inputs(case, gi)
        ads = LT.make_adapters(sd, case["rank"], case["scaling"], case["init"], seed=case["seed"])
        rdx, rg, _ = FL.adapted_fp8_grads_ref(cfg, sd, ads, x, ctx, t_mod, dout, case["grid"])
        c0 = FL.adapted_fp8_chain(cfg, sd, ads, x, ctx, t_mod, dout, case["grid"], 0, case["prescale"])
        _TAPE[name] = ((cfg, sd, x, ctx, t_mod, dout), ads, TP.with_dx(rdx, rg), TP.with_dx(c0[0], c0[1]))
    return _TAPE[name]


def _tape_block(cfg, sd, ads, rank, adapters=True):
    """A frozen enable_fp8 block with the case's trainable adapters installed (values written into the parameters' own storage)."""
    from goal_force_amd import dit, lora
    blk = dit.DiTBlock(False, cfg["dim"], cfg["num_heads"], cfg["ffn_dim"], cfg["eps"])
    blk.load_state_dict(sd, strict=True)
    blk = dit.enable_fp8(blk.to(BF).cuda())
    for p_ in blk.parameters():
        p_.requires_grad_(False)
    if adapters:
        s = next(iter(ads.values()))[0][2]
        assert lora.add_trainable(blk, TARGETS, rank, alpha=rank * s) == 10
        with torch.no_grad():
            for layer, lst in ads.items():
                (ad,) = lora.adapters(blk.get_submodule(layer))
                ad.down.copy_(lst[0][0].cuda())
                ad.up.copy_(lst[0][1].cuda())
    return blk


def _tape_run(ops, name, level=None, monkeypatch=None, adapters=True, count=None):
    from goal_force_amd import dit, lora, training
    case = TAPE_CASES[name]
    (cfg, sd, x, ctx, t_mod, dout), ads, _, _ = _tape_case(name)
    old_b, old_f = lora.set_beside_fp8(True), training.set_fp8_frozen(True)
    try:
        blk = _tape_block(cfg, sd, ads, case["rank"], adapters)
        if level is not None:
            monkeypatch.setattr(training, "KEEP_ATTENTION", True)
            monkeypatch.setattr(training, "KEEP_WIDE", False)
            monkeypatch.setattr(training, "KEEP_AUTO", True)
            training.set_keep_level(level)
        rope = dit.RopeTable.from_grid(dit.precompute_freqs_cis_3d(cfg["dim"] // cfg["num_heads"]), *case["grid"], "cuda")
        xc = x.cuda().requires_grad_(True)
        with torch.enable_grad(), ops.options(attn_q_prescale=case["prescale"]):
            y = training.block_forward(blk, xc, ctx.cuda(), t_mod.cuda(), rope)
            n_fwd = count.take() if count is not None else None
            y.backward(dout.cuda())
            if count is not None:
                count.routes = (n_fwd, count.take())
        got = {"dx": xc.grad.cpu()}
        for layer in ads:
            for i, ad in enumerate(lora.adapters(blk.get_submodule(layer))):
                assert ad.down.grad is not None and ad.up.grad is not None, f"{layer}: the adapter got no gradient"
                got[f"{layer}.lora_A.{i}"], got[f"{layer}.lora_B.{i}"] = ad.down.grad.cpu(), ad.up.grad.cpu()
        import tape_refs as TP
        named = dict(blk.named_parameters())
        assert all(named[n].grad is None for n in TP.PARAM_NAMES), "a base weight of the frozen fp8 block carries a gradient"
        return got, y.detach(), blk
    finally:
        lora.set_beside_fp8(old_b), training.set_fp8_frozen(old_f)


def _tape_rows(got, c0, ref, what):
    import lora_train_refs as LT
    import tape_refs as TP
    stats, bars = TP.measure(got, c0, ref), FL.tape_bars()
    for k, v in sorted(LT.lora_worst_by_group(stats).items()):
        print(f"ROW {what} {k}: worst ratio {v:.3f} (restatement {FL.TAPE_ROW_WORST.get(k, float('nan')):.3f}, bar {bars[k]:.3f})")
    fails = LT.lora_failures(stats, bars)
    assert not fails, f"{what}: " + "; ".join(fails)


@pytest.mark.parametrize("name", [n for n in TAPE_CASES if not n.endswith("peft")])
def test_tape_adapter_gradients_and_dx_beside_a_frozen_fp8_block(ops, name):
    """dA, dB of all ten adapters and dx, per row and per column, against fp64 autograd of the straight-through fp8 block plus peft's
    unmerged term on the unquantised input: 64 / 65 / 130 / 72 tokens, ranks 4 and 33, q pre-scale on and off."""
    _, ads, ref, c0 = _tape_case(name)
    got, _, _ = _tape_run(ops, name)
    assert set(got) == set(ref)
    _tape_rows(got, c0, ref, f"fp8 + lora tape {name}")


@pytest.mark.parametrize("level", ["none", "attn", "wide"])
def test_tape_at_520_tokens_runs_the_fused_kernel_in_the_forward_and_the_recompute(ops, level, monkeypatch):
    """520 tokens: every adapted layer that sees the tokens runs gf_gemm_fp8_lora — in the forward all eight (cross_attn.k / v see the seven
    context rows: two launches), in the backward's recompute the ones the keep level leaves to recompute (none: q, k, v, o, cross q, cross
    o with its residual form, ffn.0; ffn.2's output is read by no gradient of a frozen block; wide: cross q and ffn.0 only, the rest was
    kept) — and the gradients hold the bars."""
    name = "tiny-520-7-r33"
    _, ads, ref, c0 = _tape_case(name)
    cnt = Count(ops, monkeypatch)
    got, _, _ = _tape_run(ops, name, level=level, monkeypatch=monkeypatch, count=cnt)
    n_fwd, n_bwd = cnt.routes
    print(f"ROUTES keep={level}: forward {n_fwd}, backward {n_bwd}")
    assert n_fwd == dict(fused=8, up=2), n_fwd
    assert n_bwd["fused"] == {"none": 7, "attn": 7, "wide": 2}[level], n_bwd
    assert n_bwd["up"] == 2 + 8, n_bwd               # cross_attn.k / v recomputed by two launches; dx behind the eight token-side adapters
    _tape_rows(got, c0, ref, f"fp8 + lora tape 520 tokens keep={level}")


@pytest.mark.parametrize("level", ["none", "attn", "wide"])
def test_tape_at_every_keep_level(ops, level, monkeypatch):
    name = "tiny-65-65-r33"
    _, ads, ref, c0 = _tape_case(name)
    got, _, _ = _tape_run(ops, name, level=level, monkeypatch=monkeypatch)
    _tape_rows(got, c0, ref, f"fp8 + lora tape keep={level}")


def test_tape_peft_init_is_the_plain_fp8_block_and_dA_is_zero(ops):
    name = "tiny-64-64-peft"
    got, y, _ = _tape_run(ops, name)
    assert all(not bool(v.any()) for k, v in got.items() if ".lora_A." in k), "lora_B = 0: dA is exactly zero"
    assert any(bool(v.any()) for k, v in got.items() if ".lora_B." in k)
    _, y_plain, _ = _tape_run(ops, name, adapters=False)
    assert torch.equal(y, y_plain), "peft's init: the plain frozen fp8 block's bits"
    _, ads, ref, c0 = _tape_case(name)
    _tape_rows(got, c0, ref, "fp8 + lora tape, peft init")


def test_four_optimiser_steps_through_the_train_scripts_own_steps(ops, tmp_path):
    """scripts/train.py's steps for `--enable_fp8_training --lora_base_model dit --lora_beside_fp8` on the TINY pipeline — parser,
    check_args, the freeze, add_lora, enable_fp8_training — then four steps of launch_training_task: only the adapters move, the forward
    afterwards is that of a NEW fp8 model with the written adapters attached, and `--lora_checkpoint` restores them bit for bit."""
    import datetime
    import importlib.util
    import math
    import os
    import types
    import gen_inputs as gi
    from safetensors.torch import save_file
    from goal_force_amd import dit as D
    from goal_force_amd import lora, training
    from goal_force_amd.controlnet import ControlNet
    from goal_force_amd.pipeline import WanVideoPipeline
    spec = importlib.util.spec_from_file_location("gf_train_script_fp8_lora", os.path.join(os.path.dirname(__file__), "..", "scripts", "train.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    cfg, inp, tid = gi.TINY, gi.train_inputs(), gi.TRAIN_TIMESTEP_ID
    dit_sd, cn_sd = gi.dit_sd(cfg, seed=41), gi.controlnet_sd(cfg, 2, seed=42, zero_convs_zero=False)
    dev = {k: v.cuda() for k, v in inp.items()}

    def pipe_of():
        m = D.WanModel(has_image_input=False, require_clip_embedding=False, **cfg)
        m.load_state_dict(dit_sd, strict=True)
        cn = ControlNet(2, dim=cfg["dim"], num_heads=cfg["num_heads"], ffn_dim=cfg["ffn_dim"])
        cn.load_state_dict(cn_sd, strict=True)
        p_ = WanVideoPipeline.from_modules(m.to(BF).cuda(), None, cn.to(BF).cuda(), None, device="cuda")
        p_.scheduler.set_timesteps(1000, training=True)
        return p_

    def loss_of(p_):
        with torch.enable_grad():
            return p_.training_loss(input_latents=dev["input_latents"], noise=dev["noise"], context=dev["context"], y=dev["y"],
                                    control_signal_video_latents=dev["control"], timestep_id=tid)
    base = ["--dataset_base_path", "x", "--control_signal_type", "canny_edge", "--trainable_models", "", "--enable_fp8_training",
            "--lora_base_model", "dit", "--lora_rank", "4"]
    with pytest.raises(NotImplementedError, match="trainable LoRA adapters run on bf16 layers only"):
        script.check_args(script.parser().parse_args(base))
    old_b, old_f = lora.beside_fp8(), training.FP8_FROZEN
    try:
        cli = script.parser().parse_args(base + ["--lora_beside_fp8"])
        script.check_args(cli)
        pipe = pipe_of()
        pipe.freeze_except([])
        script.add_lora(pipe, cli)
        assert lora.beside_fp8() is True and len(lora.trainable(pipe.dit)) == 10 * cfg["num_layers"]
        assert script.enable_fp8_training(pipe, cli) == 1 and training.FP8_FROZEN is True
        assert all(D.precision(b.ffn[0]) == "fp8" for b in pipe.dit.blocks)
        args = types.SimpleNamespace(learning_rate=1e-3, weight_decay=1e-2, dataset_num_workers=0, save_steps=None, num_epochs=1,
                                     gradient_accumulation_steps=1, output_path=str(tmp_path), remove_prefix_in_ckpt="pipe.dit.",
                                     control_signal_type="canny_edge", num_frames=5, max_grad_norm=1.0, controlnet_checkpoint=None)
        control = torch.zeros(5, 480, 832, 3, dtype=torch.uint8)
        items = [dict(video=[], control_video=control, file_id=str(i)) for i in range(4)]
        lora_ids = {id(p_) for p_ in lora.trainable_parameters(pipe.dit)}
        before = {n: p_.detach().clone() for m in (pipe.dit, pipe.controlnet) for n, p_ in m.named_parameters()}
        seen = []

        def forward(p_, data):
            seen.append(loss_of(p_))
            return seen[-1]
        logger = training.launch_training_task(items, pipe, args=args, forward=forward, shuffle=False, now=datetime.datetime(2026, 1, 2, 3, 4, 5))
        assert logger.num_steps == 4 and all(math.isfinite(float(v.detach())) for v in seen)
        moved = {n for m in (pipe.dit, pipe.controlnet) for n, p_ in m.named_parameters() if not torch.equal(before[n], p_.detach())}
        assert moved and all(".lora_A." in n or ".lora_B." in n for n in moved), sorted(moved)[:4]
        assert any(".lora_B." in n for n in moved), "lora_B left its zero initialisation"
        assert all(p_.grad is None for m in (pipe.dit, pipe.controlnet) for p_ in m.parameters() if id(p_) not in lora_ids)
        from goal_force_amd.model_fn import model_fn_wan_video
        tin = {k: v.cuda() for k, v in gi.tiny_inputs().items()}

        def fwd(model):        # the inference forward (the tape refuses a frozen attached adapter, as on bf16 blocks)
            with torch.no_grad():
                return model_fn_wan_video(model, latents=tin["latents"], timestep=torch.tensor([995.9], dtype=BF).cuda(), context=tin["ctx_posi"],
                                          y=tin["y"]).clone()
        trained = fwd(pipe.dit)
        sd = lora.trainable_state_dict(pipe.dit)
        path = str(tmp_path / "adapters.safetensors")
        save_file({k: v.contiguous().cpu() for k, v in sd.items()}, path)
        # a NEW fp8 model with the written adapters attached: the same forward
        fresh = pipe_of()
        fresh.freeze_except([])
        D.enable_fp8(fresh.dit)
        assert lora.attach(fresh.dit, sd, alpha=1.0) == 10 * cfg["num_layers"]
        assert torch.equal(fwd(fresh.dit), trained)
        # --lora_checkpoint round-trips
        again = pipe_of()
        again.freeze_except([])
        script.add_lora(again, script.parser().parse_args(base + ["--lora_beside_fp8", "--lora_checkpoint", path]))
        script.enable_fp8_training(again, cli)
        sd2 = lora.trainable_state_dict(again.dit)
        assert sorted(sd2) == sorted(sd) and all(torch.equal(sd2[k], sd[k]) for k in sd)
        assert torch.equal(fwd(again.dit), trained)
    finally:
        lora.set_beside_fp8(old_b), training.set_fp8_frozen(old_f)
