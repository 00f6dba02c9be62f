"""The LoRA kernels per element through the raw C ABI (gf_lora_merge, gf_lora_up: goal_force_amd/csrc/gf_lora.hip), and the two forms
on modules (pipe.load_lora / lora.attach).  The chain, the bars and the inputs are tests/lora_refs.py's; tests/test_lora_cpu.py shows
that the fp32 restatement passes the bars on every gauss input used here and that each stated fault does not.

Per element: the exact classes (selector: every delta is one scaled element of the column factor; integers) with torch.equal, the
activation epilogues of gf_lora_up held to gf_act of the exact y as tests/test_gemm_pinned_gpu.py does; gauss through gemm_refs'
two bars with K = the rank.  Every kernel call here writes into a strided view inside a guarded parent and reads operands with NaN
in their gaps and behind them."""
import os

import numpy as np
import pytest
import torch

import forward_refs as FR
import gemm_refs as G
import lora_refs as LR

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENT = 0x5A5A
GF_ERR_INVALID_ARG = -1
KINDS = {G.EPI_GELU: "gelu_tanh", G.EPI_SILU: "silu"}
CLASSES = ("selector", "integers", "gauss")
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
def _no_grad():
    with torch.no_grad():
        yield


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16)


def _err(lib):
    return lib.gf_last_error().decode()


class Held:
    """A [rows, cols] bf16 operand as a strided view (row pitch ld) inside a parent: 8 elements in front, the rows' gaps and 64 elements
    behind hold `fill` — NaN for what a kernel reads (a read outside the operand poisons the result), the sentinel for what it
    writes (a write outside shows)."""

    def __init__(self, t, ld, fill="nan", front=8):
        rows, cols = t.shape
        assert ld >= cols
        self.n = front + rows * ld + 64
        self.parent = torch.empty(self.n, dtype=BF, device="cuda")
        if fill == "nan":
            self.parent.fill_(float("nan"))
        else:
            self.parent.view(torch.int16).fill_(SENT)
        self.view = self.parent[front:front + rows * ld].view(rows, ld)[:, :cols] if rows else self.parent[front:front].view(0, cols)
        self.view.copy_(t.cuda())
        self.mask = torch.ones(self.n, dtype=torch.bool, device="cuda")
        if rows:
            self.mask[front:front + rows * ld].view(rows, ld)[:, :cols] = False
        self.before = self.parent.view(torch.int16).clone()
        self.ld = ld

    def guards_intact(self):
        return bool((self.parent.view(torch.int16)[self.mask] == self.before[self.mask]).all())

    def untouched(self):
        return bool((self.parent.view(torch.int16) == self.before).all())


def _note(kind, j):
    f = FIG.setdefault(kind, dict(n=0, share=0.0, worst=0.0))
    f["n"] += 1
    f["share"], f["worst"] = max(f["share"], j["share"]), max(f["worst"], j["worst"])


def _where(diff, d=None):
    idx = torch.nonzero(diff)
    first = idx[:6].tolist()
    extra = ""
    if d is not None and "j" in d and first:
        extra = "; (row, rank column of its selector): " + str([(r, int(d["j"][r])) for r, _ in first])
    return f"{idx.shape[0]} elements differ; first (row, column): {first}{extra}"


# ---------------------------------------------------------------------------------------------------------------------
# gf_lora_merge
def _merge(lib, W, up, down, n, k, r, alpha, ldw=None, ld_up=None, ld_down=None):
    return lib.gf_lora_merge(W if isinstance(W, int) or W is None else W.data_ptr(), ldw, None if up is None else (up if isinstance(up, int) else up.data_ptr()),
                             ld_up, None if down is None else (down if isinstance(down, int) else down.data_ptr()), ld_down, n, k, r, alpha, _st())


def _merge_held(lib, d, aligned):
    """One merge of an input dict in guarded surroundings -> (result on the CPU, the three Held).  `aligned`: up / down with pitches
    that are multiples of 8 (the kernel's 16-byte reads of the factors); otherwise odd pitches (its element reads)."""
    n, k = d["w"].shape
    r = d["up"].shape[1]
    W = Held(d["w"], k + 8, fill="sentinel")
    up = Held(d["up"], (-(-r // 8) * 8 + 8) if aligned else r + 3)
    down = Held(d["down"], k + 8 if aligned else k + 5)
    rc = _merge(lib, W.view, up.view, down.view, n, k, r, d["alpha"], W.ld, up.ld, down.ld)
    torch.cuda.synchronize()
    assert rc == 0, _err(lib)
    assert W.guards_intact(), "gf_lora_merge wrote outside W"
    assert up.untouched() and down.untouched()
    return W.view.cpu(), (W, up, down)


def _check_merge(got, d, cls, what):
    ref = LR.merge_chain(d)
    if cls == "gauss":
        _note("merge", G.assert_pinned(got, ref, d["rank"], what))
        return
    diff = _bits(got) != _bits(ref.out.to(BF))
    print(f"PIN {what}: equal to the chain {not bool(diff.any())}")
    assert not bool(diff.any()), f"{what}: exact operands, so any difference is a fault: {_where(diff, d)}"


@pytest.mark.parametrize("n,k,r,alpha", LR.MERGE_CASES)
def test_merge_tile_edges_three_classes(lib, n, k, r, alpha):
    for cls in CLASSES:
        d = LR.merge_inputs(cls, n, k, r, alpha)
        for aligned in (True, False):
            got, _ = _merge_held(lib, d, aligned)
            _check_merge(got, d, cls, f"merge {cls} {(n, k, r, alpha)} {'16-byte' if aligned else 'element'} factor reads")


def test_merge_through_the_wrapper_bumps_the_version_and_stacks(ops):
    d = LR.merge_inputs("integers", 65, 72, 33, 0.7)
    w = torch.nn.Parameter(d["w"].cuda())
    v0 = w._version
    assert ops.lora_merge(w, d["up"].cuda(), d["down"].cuda(), d["alpha"]) is w and w._version > v0
    once = LR.merge_chain(d).out.to(BF)
    assert torch.equal(_bits(w.detach().cpu()), _bits(once))
    ops.lora_merge(w, d["up"].cuda(), d["down"].cuda(), d["alpha"])             # twice applies the delta twice
    twice = LR.merge_chain(dict(d, w=once)).out.to(BF)
    assert torch.equal(_bits(w.detach().cpu()), _bits(twice)) and not torch.equal(once, twice)


def test_merge_no_rows_and_refusals_leave_w_untouched(ops, lib):
    d = LR.merge_inputs("integers", 17, 24, 4, 1.0)
    W, up, down = Held(d["w"], 32, fill="sentinel"), Held(d["up"], 8), Held(d["down"], 32)
    assert _merge(lib, W.view, up.view, down.view, 0, 24, 4, 1.0, 32, 8, 32) == 0
    torch.cuda.synchronize()
    assert W.untouched()
    p = W.view.data_ptr()
    bad = [
        (dict(k=20), "k_in=20 must be a multiple of 8"),
        (dict(ldw=28), "ldw=28 must be a multiple of 8"),
        (dict(ldw=16), "ldw=16 must be a multiple of 8 and cover the row"),
        (dict(W=p + 2), "16-byte alignment of W"),
        (dict(W=None), "null pointer"), (dict(up=None), "null pointer"), (dict(down=None), "null pointer"),
        (dict(r=0), "rank=0 outside 1..256"), (dict(r=257, ld_up=264), "rank=257 outside 1..256"),
        (dict(ld_up=3), "ld_up / ld_down must cover the row"), (dict(ld_down=23), "ld_up / ld_down must cover the row"),
        (dict(up=up.view.data_ptr() + 1), "2-byte aligned"),
        (dict(alpha=float("nan")), "alpha must be finite"), (dict(alpha=float("inf")), "alpha must be finite"),
        (dict(n=-1), "bad shape"), (dict(k=0), "bad shape"),
        (dict(n=(1 << 30) - 1, k=(1 << 30) - 8, ldw=(1 << 30) - 8, ld_down=(1 << 30) - 8), "exceed the grid"),   # 2^24 x 2^24 tiles
    ]
    for change, msg in bad:
        a = dict(W=p, up=up.view.data_ptr(), down=down.view.data_ptr(), n=17, k=24, r=4, alpha=1.0, ldw=32, ld_up=8, ld_down=32)
        a.update(change)
        rc = _merge(lib, a["W"], a["up"], a["down"], a["n"], a["k"], a["r"], a["alpha"], a["ldw"], a["ld_up"], a["ld_down"])
        assert rc == GF_ERR_INVALID_ARG and msg in _err(lib), (change, rc, _err(lib))
    torch.cuda.synchronize()
    assert W.untouched()
    # the wrapper's own words
    from goal_force_amd._lib import GoalForceError
    w = d["w"].cuda()
    keep = w.clone()
    for args, msg in [((w, d["up"][:16].cuda(), d["down"].cuda()), r"expected up \[17, r\]"), ((w, d["up"].cuda(), d["down"][:, :16].cuda()), r"down \[r, 24\]"),
                      ((w, d["up"].cuda().float(), d["down"].cuda()), "expected dtype"), ((w, d["up"], d["down"].cuda()), "must be on the GPU"),
                      ((w.t(), d["up"].cuda(), d["down"].cuda()), "contiguous rows")]:
        with pytest.raises(GoalForceError, match=msg):
            ops.lora_merge(*args)
    with pytest.raises(GoalForceError, match="alpha must be finite"):
        ops.lora_merge(w, d["up"].cuda(), d["down"].cuda(), float("nan"))
    assert torch.equal(w, keep)


def test_load_refuses_a_layer_the_kernel_would_refuse_before_the_first_write():
    """in_features not a multiple of 8: refused by name in lora.load's own pass over the layers, the layer ahead of it unwritten."""
    from goal_force_amd import lora
    from goal_force_amd._lib import GoalForceError
    net = torch.nn.Sequential(torch.nn.Linear(16, 8), torch.nn.Linear(12, 8)).to(BF).cuda()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    sd = {"0.lora_B.weight": torch.ones(8, 4), "0.lora_A.weight": torch.ones(4, 16), "1.lora_B.weight": torch.ones(8, 4), "1.lora_A.weight": torch.ones(4, 12)}
    with pytest.raises(GoalForceError, match=r"load_lora: '1': gf_lora_merge takes a weight with contiguous rows, in_features and row pitch multiples of 8"):
        lora.load(net, sd)
    torch.cuda.synchronize()
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    assert lora.load(net, {k: v for k, v in sd.items() if k.startswith("0.")}) == 1
    assert not torch.equal(net[0].weight, before["0.weight"]) and torch.equal(net[1].weight, before["1.weight"])


@pytest.mark.parametrize("cls", LR.GOLDEN_CLASSES)
def test_merge_against_the_references_loader(ops, cls):
    """g21: the reference's GeneralLoRALoader in bf16 on the CPU, two stacked loads on the tiny expert."""
    from conftest import GOLDEN
    g21 = np.load(os.path.join(GOLDEN, "g21_lora.npz"))
    refs, _, dicts = LR.golden_reference_weights(g21, cls)
    base = LR.golden_base_sd(cls)
    w = {n: base[n + ".weight"].cuda() for n in LR.GOLDEN_TARGETS}
    worst = 0.0
    for load, (_, _, _, alpha) in enumerate(LR.GOLDEN_LOADS):
        lsd = LR.golden_lora_sd(load, cls, base)
        for n in LR.GOLDEN_TARGETS:
            kb, ka = dicts[load][n]
            w[n].copy_(refs[load - 1][n] if load else base[n + ".weight"])        # every load starts from what the REFERENCE left
            ops.lora_merge(w[n], lsd[kb].cuda(), lsd[ka].cuda(), alpha)
            got, ref = w[n].cpu(), refs[load][n]
            diff = _bits(got) != _bits(ref)
            if cls == "integers":
                assert not bool(diff.any()), f"g21 integers load {load} {n}: {_where(diff)}"
            else:
                share = float(diff.double().mean())
                worst = max(worst, share)
                assert share <= 2.0 ** -10 and int(FR.bf16_steps(got, ref).max()) <= 1, f"g21 gauss load {load} {n}: share {share:.2e}"
    print(f"PIN g21 {cls}: worst share of elements that differ from the reference's result {worst:.2e} (cap 2^-10; the reference's own "
          f"distance from the chain on the CPU: {float(g21['cpu_share']):.2e})")


# ---------------------------------------------------------------------------------------------------------------------
# gf_lora_up
def _up(lib, y0, ldy, t, ldt, up, ld_up, out, ldo, M, N, R, scale, epi, resid=None, ldr=0, gate=None):
    p = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())          # noqa: E731
    return lib.gf_lora_up(p(y0), ldy, p(t), ldt, p(up), ld_up, p(out), ldo, M, N, R, scale, epi, p(resid), ldr, p(gate), _st())


def _up_held(lib, d, epi, alias=None):
    """One call in guarded surroundings -> the result on the CPU.  alias: None (out a buffer of its own), "y0" or "resid"."""
    M, N = d["y0"].shape
    R = d["t"].shape[1]
    y0 = Held(d["y0"], N + 8, fill="sentinel" if alias == "y0" else "nan")
    t, up = Held(d["t"], R + 8), Held(d["up"], R + 16)
    has_r = epi in LR.HAS_R
    resid = Held(d["resid"], N + 16, fill="sentinel" if alias == "resid" else "nan") if has_r else None
    gate = d["gate"].cuda() if epi == G.EPI_GATE_RESID else None
    out = {"y0": y0, "resid": resid}.get(alias) or Held(torch.zeros((M, N), dtype=BF), N + 24, fill="sentinel")
    rc = _up(lib, y0.view, y0.ld, t.view, t.ld, up.view, up.ld, out.view, out.ld, M, N, R, d["scale"], epi,
             resid.view if has_r else None, resid.ld if has_r else 0, gate)
    torch.cuda.synchronize()
    assert rc == 0, _err(lib)
    assert out.guards_intact(), "gf_lora_up wrote outside out"
    for h in (y0, t, up, resid):
        assert h is None or h is out or h.untouched()
    return out.view.cpu()


def _check_up(ops, got, d, cls, epi, what):
    ref, y = LR.up_chain(d, epi)
    if cls == "gauss":
        _note("up", G.assert_pinned(got, ref, d["t"].shape[1], what))
        return
    if epi in KINDS:             # the exact y through gf_act, bit for bit; and within one bf16 step of bf16(fp64 function)
        yb = y.to(BF)
        want = torch.where(G.tail_mask(yb, epi), torch.full_like(yb, -0.0), ops.act(yb.cuda(), KINDS[epi]).cpu())
        bad = _bits(got) != _bits(want)
        assert not bool(bad.any()), f"{what}: not gf_act of the exact y: {_where(bad, d)}"
        assert int(FR.bf16_steps(got, ref.out.to(BF)).max()) <= 1, what
    else:
        diff = _bits(got) != _bits(ref.out.to(BF))
        assert not bool(diff.any()), f"{what}: exact operands, so any difference is a fault: {_where(diff, d)}"


@pytest.mark.parametrize("M,N,rp,r,scale", LR.UP_CASES)
def test_up_tile_edges_three_classes_six_epilogues(ops, lib, M, N, rp, r, scale):
    for cls in CLASSES:
        d = LR.up_inputs(cls, M, N, rp, r, scale)
        for epi in G.EPIS:
            _check_up(ops, _up_held(lib, d, epi), d, cls, epi, f"up {cls} {(M, N, rp, r, scale)} {G.EPI_NAMES[epi]}")


@pytest.mark.parametrize("M,N,rp,r,scale", [(129, 136, 64, 33, 0.7), (65, 72, 32, 1, 1.0)])
def test_up_out_aliases_y0_or_resid(ops, lib, M, N, rp, r, scale):
    for cls in CLASSES:
        d = LR.up_inputs(cls, M, N, rp, r, scale)
        for epi in G.EPIS:
            _check_up(ops, _up_held(lib, d, epi, alias="y0"), d, cls, epi, f"up out=y0 {cls} {G.EPI_NAMES[epi]}")
            if epi in LR.HAS_R:
                _check_up(ops, _up_held(lib, d, epi, alias="resid"), d, cls, epi, f"up out=resid {cls} {G.EPI_NAMES[epi]}")


def test_up_through_the_wrapper(ops):
    d = LR.up_inputs("integers", 130, 72, 64, 33, 0.7)
    dev = {k: v.cuda() for k, v in d.items() if torch.is_tensor(v)}
    for epi in (G.EPI_BIAS, G.EPI_GATE_RESID, G.EPI_MUL):
        out = ops.lora_up(dev["y0"], dev["t"], dev["up"], d["scale"], epilogue=epi, resid=dev["resid"] if epi in LR.HAS_R else None,
                          gate=dev["gate"] if epi == G.EPI_GATE_RESID else None)
        assert torch.equal(_bits(out.cpu()), _bits(LR.up_chain(d, epi)[0].out.to(BF)))
    y = dev["y0"].clone()
    assert ops.lora_up(y, dev["t"], dev["up"], d["scale"], out=y) is y
    assert torch.equal(_bits(y.cpu()), _bits(LR.up_chain(d, 0)[0].out.to(BF)))


def test_up_no_rows_and_refusals_leave_out_untouched(ops, lib):
    d = LR.up_inputs("integers", 17, 24, 32, 4, 1.0)
    y0, t, up = Held(d["y0"], 32), Held(d["t"], 40), Held(d["up"], 40)
    resid, out = Held(d["resid"], 32), Held(torch.zeros((17, 24), dtype=BF), 32, fill="sentinel")
    gate = d["gate"].cuda()
    base = dict(y0=y0.view.data_ptr(), ldy=32, t=t.view.data_ptr(), ldt=40, up=up.view.data_ptr(), ld_up=40, out=out.view.data_ptr(), ldo=32,
                M=17, N=24, R=32, scale=1.0, epi=2, resid=resid.view.data_ptr(), ldr=32, gate=gate.data_ptr())
    assert _up(lib, **dict(base, M=0)) == 0
    bad = [
        (dict(N=20), "N=20 must be a multiple of 8"), (dict(R=16), "rank_pad=16"), (dict(R=288), "rank_pad=288"), (dict(R=40), "rank_pad=40"),
        (dict(ldy=28), "leading dimensions"), (dict(ldo=16), "leading dimensions"), (dict(ldt=24), "leading dimensions"), (dict(ld_up=36), "leading dimensions"),
        (dict(y0=base["y0"] + 2), "16-byte alignment"), (dict(out=base["out"] + 2), "16-byte alignment"), (dict(t=None), "null pointer"),
        (dict(scale=float("nan")), "scale must be finite"), (dict(epi=6), "unknown epilogue 6"), (dict(epi=-1), "unknown epilogue -1"),
        (dict(resid=None), "residual epilogue needs"), (dict(ldr=20), "residual epilogue needs"), (dict(gate=None), "gate epilogue needs"),
        (dict(epi=5, resid=None), "residual epilogue needs"), (dict(M=-1), "bad shape"),
    ]
    for change, msg in bad:
        rc = _up(lib, **dict(base, **change))
        assert rc == GF_ERR_INVALID_ARG and msg in _err(lib), (change, rc, _err(lib))
    torch.cuda.synchronize()
    assert out.untouched()
    from goal_force_amd._lib import GoalForceError
    dev = {k: v.cuda() for k, v in d.items() if torch.is_tensor(v)}
    for kw, msg in [(dict(t=dev["t"][:16]), r"lora_up\.t: expected \[17, 32\]"), (dict(up=dev["up"][:16]), r"lora_up\.up: expected \[24, 32\]"),
                    (dict(t=dev["t"][:, :16].contiguous(), up=dev["up"][:, :16].contiguous()), "padded rank 16"),
                    (dict(scale=float("inf")), "scale must be finite"), (dict(out=torch.empty(17, 16, dtype=BF, device="cuda")), r"expected \[17, 24\]")]:
        a = dict(y0=dev["y0"], t=dev["t"], up=dev["up"], scale=1.0)
        a.update(kw)
        with pytest.raises(GoalForceError, match=msg):
            ops.lora_up(**a)


# ---------------------------------------------------------------------------------------------------------------------
# modules
LAYERS = tuple(f"{a}.{p}" for a in ("self_attn", "cross_attn") for p in "qkvo") + ("ffn.0", "ffn.2")
WIDTHS = {"mid": (1536, 12, 8960), "a14b": (5120, 40, 13824)}
GRIDS = {64: (1, 8, 8), 65: (1, 5, 13), 130: (2, 5, 13)}
CTX = 48          # 40 distinct context rows and a run of 8 identical ones: the cross-attention folds its keys (and, inference, o)
_MOD = {}


def _adapter_sd(sd, layers, rank, seed, spelling="lora_B.weight", prefix=""):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in layers:
        n, k = sd[name + ".weight"].shape
        out[f"{prefix}{name}.{spelling}"] = (torch.randn((n, rank), generator=g) / k ** 0.5).to(BF)
        out[f"{prefix}{name}.{spelling}".replace("lora_B", "lora_A")] = (torch.randn((rank, k), generator=g) / rank ** 0.5).to(BF)
    return out


def _setup(width, tokens):
    """(state dict, inputs on the device, oracle inputs) of one block shape, built once."""
    key = (width, tokens)
    if key not in _MOD:
        import gen_inputs as gi
        from goal_force_amd.dit import RopeTable, precompute_freqs_cis_3d
        from oracle import wan_oracle as wo
        dim, heads, ffn = WIDTHS[width]
        if width == "a14b":             # 350 M weights: drawn on the device (gen_inputs.block_sd's distributions), seconds saved per test
            g = torch.Generator(device="cuda").manual_seed(211)
            sd = {}
            for name, shp in wo.block_param_shapes(dim, ffn).items():
                t = torch.randn(shp, generator=g, device="cuda")
                if name.endswith(("norm_q.weight", "norm_k.weight")) or name == "norm3.weight":
                    t = 1.0 + 0.1 * t
                else:
                    t = t * (0.02 if name.endswith(".bias") else (1.0 / dim ** 0.5 if name == "modulation" else 1.0 / shp[1] ** 0.5))
                sd[name] = t.to(BF).cpu()
        else:
            sd = gi.block_sd(torch.Generator().manual_seed(211), dim, ffn, "", BF)
        x, ctx, t_mod = gi.block_inputs(dim, tokens, CTX, seed=212)
        ctx[0, 40:] = ctx[0, 40]
        rope = RopeTable.from_grid(precompute_freqs_cis_3d(128), *GRIDS[tokens], "cuda")
        _MOD[key] = dict(sd=sd, sd_dev={k: v.cuda() for k, v in sd.items()}, dev=(x.cuda(), ctx.cuda(), t_mod.cuda(), rope), cpu=(x, ctx, t_mod, wo.rope_freqs_3d(128, *GRIDS[tokens])),
                         shape=(dim, heads, ffn))
    return _MOD[key]


def _block(s):
    from goal_force_amd.dit import DiTBlock
    dim, heads, ffn = s["shape"]
    with torch.device("cuda"):          # built on the device: at the A14B width the host-side initialisation of 350 M weights is seconds
        blk = DiTBlock(False, dim, heads, ffn, 1e-6)
    blk = blk.to(BF)
    blk.load_state_dict(s["sd_dev"], strict=True)
    return blk


def _pipe():
    from goal_force_amd.pipeline import WanVideoPipeline
    return WanVideoPipeline.from_modules(None)


def _oracle(s, sd64):
    from oracle import wan_oracle as wo
    x, ctx, t_mod, freqs = s["cpu"]
    return wo.dit_block(x.double(), ctx.double(), t_mod.double(), freqs, sd64, "", s["shape"][1])


def _rel(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("width,tokens", [("mid", 64), ("mid", 65), ("mid", 130), ("a14b", 65)])
def test_merged_block_equals_a_block_loaded_with_the_merged_weights(width, tokens, tmp_path):
    """The caches' proof: a block that ran before the merge (and so holds whatever it derives from its weights) gives, after
    pipe.load_lora, the bits of a NEW block that load_state_dict gave the merged weights — in bf16, under enable_fp8 and under
    enable_fp4; a .safetensors path equals the state-dict call."""
    from goal_force_amd import dit
    from safetensors.torch import save_file
    s = _setup(width, tokens)
    lsd = _adapter_sd(s["sd"], LAYERS, 16, 301, "lora_B.default.weight", "diffusion_model.")
    pipe = _pipe()
    merged = None
    for mode in ("bf16", "fp8", "fp4", "file"):
        blk = _block(s)
        if mode in ("fp8", "fp4"):
            getattr(dit, "enable_" + mode)(blk)
        before = blk(*s["dev"]).clone()
        if mode == "file":
            path = str(tmp_path / "adapter.safetensors")
            save_file({k: v.contiguous() for k, v in lsd.items()}, path)
            assert pipe.load_lora(blk, path, alpha=0.7) == len(LAYERS)
        else:
            assert pipe.load_lora(blk, lsd, alpha=0.7) == len(LAYERS)
        got = blk(*s["dev"]).clone()
        assert not torch.equal(got, before)
        state = {k: v.detach().clone() for k, v in blk.state_dict().items()}
        if merged is None:
            merged = state
            for n in LAYERS:              # the weights are the chain's (per element: the kernel tests above); torch's fp64 on the device
                want = LR.merged_weight(s["sd_dev"][n + ".weight"], lsd[f"diffusion_model.{n}.lora_B.default.weight"].cuda(),
                                        lsd[f"diffusion_model.{n}.lora_A.default.weight"].cuda(), 0.7)
                share = float((_bits(state[n + ".weight"]) != _bits(want)).double().mean())
                assert share <= 2.0 ** -10, (n, share)
        else:
            assert all(torch.equal(state[k], merged[k]) for k in merged), "the merged weights do not depend on the block's mode"
        fresh = _block(s)
        fresh.load_state_dict(state, strict=True)
        if mode in ("fp8", "fp4"):
            getattr(dit, "enable_" + mode)(fresh)
        assert torch.equal(blk(*s["dev"]), fresh(*s["dev"])), f"{mode}: a copy derived from the old weights survived the merge"
        assert torch.equal(got, fresh(*s["dev"]))


def _count_launches(ops, fn):
    ops.PROFILE_GEMM = []
    try:
        out = fn().clone()
        return out, len(ops.PROFILE_GEMM)
    finally:
        ops.PROFILE_GEMM = None


@pytest.mark.parametrize("width,tokens", [("mid", 64), ("mid", 65), ("mid", 130), ("a14b", 65)])
def test_attached_block(ops, width, tokens):
    """Strength 0 and detached: the plain block's bits and launches.  Attached at 0.7: no further from the fp64 statement of peft's
    forward than 1.25 x the merged block is from the fp64 merged forward.  Two stacked adapters: their sequential application."""
    from goal_force_amd import lora
    s = _setup(width, tokens)
    # (at the A14B width one layer of each shape — D->D on both attentions, D->F, F->D: the fp64 side of 350 M weights is the test's time)
    layers = LAYERS if width != "a14b" else ("self_attn.q", "cross_attn.o", "ffn.0", "ffn.2")
    lsd = _adapter_sd(s["sd"], layers, 16, 301)
    blk = _block(s)
    plain, n_plain = _count_launches(ops, lambda: blk(*s["dev"]))
    assert lora.attach(blk, lsd, alpha=0.0) == len(layers)
    zero, n_zero = _count_launches(ops, lambda: blk(*s["dev"]))
    assert torch.equal(zero, plain) and n_zero == n_plain
    assert lora.set_strength(blk, 0.7) == len(layers)
    att, n_att = _count_launches(ops, lambda: blk(*s["dev"]))
    assert not torch.equal(att, plain) and n_att > n_plain
    assert lora.detach(blk) == len(layers)
    off, n_off = _count_launches(ops, lambda: blk(*s["dev"]))
    assert torch.equal(off, plain) and n_off == n_plain
    assert all(torch.equal(v, s["sd"][k].cuda()) for k, v in blk.state_dict().items()), "the masters are never written"
    # fp64: peft's forward is the block on W + alpha up down (unrounded); the merged forward is the block on the merged bf16 weights
    sd_peft = {k: v.double() for k, v in s["sd"].items()}
    sd_merged = dict(sd_peft)
    for n in layers:
        up, down = lsd[n + ".lora_B.weight"], lsd[n + ".lora_A.weight"]
        sd_peft[n + ".weight"] = sd_peft[n + ".weight"] + LR.f32(0.7) * (up.double() @ down.double())
        sd_merged[n + ".weight"] = LR.merged_weight(s["sd"][n + ".weight"], up, down, 0.7).double()
    mblk = _block(s)
    _pipe().load_lora(mblk, lsd, alpha=0.7)
    e_att, e_mer = _rel(att, _oracle(s, sd_peft)), _rel(mblk(*s["dev"]), _oracle(s, sd_merged))
    print(f"PIN attached block {width} {tokens} tokens: rel-L2 from fp64 peft {e_att:.3e}; merged block from the fp64 merged forward {e_mer:.3e}")
    assert e_att <= 1.25 * e_mer, (e_att, e_mer)
    # two stacked adapters = their sequential application (each in turn, in attach order), layer by layer
    lsd2 = _adapter_sd(s["sd"], ("ffn.0", "self_attn.q"), 33, 302)
    lora.attach(blk, lsd, alpha=0.7, name="a")
    lora.attach(blk, lsd2, alpha=-0.5, name="b")
    from goal_force_amd import dit
    x2 = s["dev"][0][0]
    lin = blk.ffn[0]
    a, b = lora.adapters(lin)
    got = dit.linear(x2, lin, epilogue=ops.EPI_BIAS_GELU_TANH)
    y = ops.gemm(x2, lin.weight, lin.bias)
    y = ops.lora_up(y, ops.gemm(x2, a.down), a.up, 0.7)
    y = ops.lora_up(y, ops.gemm(x2, b.down), b.up, -0.5, epilogue=ops.EPI_BIAS_GELU_TANH)
    assert torch.equal(got, y)
    both = blk(*s["dev"]).clone()
    lora.detach(blk, "b")
    assert torch.equal(blk(*s["dev"]), att) and not torch.equal(both, att)


@pytest.mark.parametrize("layer", ["self_attn.v", "cross_attn.o"])
def test_adapter_on_v_or_cross_o_takes_the_plain_path_and_meets_the_bar(ops, layer, monkeypatch):
    """2304 tokens: the plain block writes V through gf_linear_vt32 and folds the cross-attention's o into its values."""
    from goal_force_amd import dit, lora
    import gen_inputs as gi
    from oracle import wan_oracle as wo
    dim, heads, ffn = WIDTHS["mid"]
    grid, tokens = (4, 24, 24), 2304
    sd = gi.block_sd(torch.Generator().manual_seed(211), dim, ffn, "", BF)
    x, ctx, t_mod = gi.block_inputs(dim, tokens, CTX, seed=213)
    ctx[0, 40:] = ctx[0, 40]
    s = dict(sd=sd, sd_dev={k: v.cuda() for k, v in sd.items()}, shape=(dim, heads, ffn), cpu=(x, ctx, t_mod, wo.rope_freqs_3d(128, *grid)),
             dev=(x.cuda(), ctx.cuda(), t_mod.cuda(), dit.RopeTable.from_grid(dit.precompute_freqs_cis_3d(128), *grid, "cuda")))
    blk = _block(s)
    seen = []
    real_vt, real_fold = ops.linear_vt32, ops.cross_fold_table
    monkeypatch.setattr(ops, "linear_vt32", lambda *a, **k: (seen.append("vt"), real_vt(*a, **k))[1])
    monkeypatch.setattr(ops, "cross_fold_table", lambda *a, **k: (seen.append("fold"), real_fold(*a, **k))[1])
    blk(*s["dev"])
    assert "vt" in seen and "fold" in seen, f"the plain block took neither special path ({seen}): the test shows nothing"
    lsd = _adapter_sd(sd, (layer,), 16, 303)
    lora.attach(blk, lsd, alpha=0.7)
    del seen[:]
    att = blk(*s["dev"]).clone()
    assert ("vt" if layer == "self_attn.v" else "fold") not in seen
    up, down = lsd[layer + ".lora_B.weight"], lsd[layer + ".lora_A.weight"]
    sd_peft = {k: v.double() for k, v in sd.items()}
    sd_merged = dict(sd_peft)
    sd_peft[layer + ".weight"] = sd_peft[layer + ".weight"] + LR.f32(0.7) * (up.double() @ down.double())
    sd_merged[layer + ".weight"] = LR.merged_weight(sd[layer + ".weight"], up, down, 0.7).double()
    mblk = _block(s)
    _pipe().load_lora(mblk, lsd, alpha=0.7)
    e_att, e_mer = _rel(att, _oracle(s, sd_peft)), _rel(mblk(*s["dev"]), _oracle(s, sd_merged))
    print(f"PIN adapter on {layer}: rel-L2 from fp64 peft {e_att:.3e}; merged block from the fp64 merged forward {e_mer:.3e}")
    assert e_att <= 1.25 * e_mer, (e_att, e_mer)


def test_refusals_of_the_attached_form():
    from goal_force_amd import dit, lora
    from goal_force_amd._lib import GoalForceError
    s = _setup("mid", 64)
    lsd = _adapter_sd(s["sd"], ("ffn.0", "self_attn.q"), 4, 304)
    blk = _block(s)
    dit.enable_fp8(blk)
    with pytest.raises(GoalForceError, match=r"lora\.attach: 'self_attn\.q' carries an enable_fp8 weight copy"):
        lora.attach(blk, lsd)
    dit.enable_fp8(blk, False)
    dit.enable_fp4(blk)
    with pytest.raises(GoalForceError, match=r"lora\.attach: 'ffn\.0' carries an enable_fp4 weight copy"):
        lora.attach(blk, {k: v for k, v in lsd.items() if "ffn" in k})
    dit.enable_fp4(blk, False)
    assert lora.attach(blk, lsd) == 2
    for enable, kind in ((dit.enable_fp8, "fp8"), (dit.enable_fp4, "fp4")):
        enable(blk)
        with pytest.raises(GoalForceError, match=f"an attached LoRA adapter \\('default'\\) on an enable_{kind} layer is refused"):
            blk(*s["dev"])
        enable(blk, False)
    x2 = s["dev"][0][0]
    with pytest.raises(GoalForceError, match="a QuantizedInput was handed to or asked of a layer with an attached LoRA adapter"):
        dit.linear(dit.QuantizedInput(x2), blk.ffn[0])
    with pytest.raises(GoalForceError, match="training through a block with a live LoRA adapter"):
        dit.refuse_training(blk)
    lora.detach(blk)
    dit.refuse_training(blk)


def test_a_context_cache_kept_across_a_change_empties_itself():
    """One ContextCache handed to model_fn before and after lora.attach / set_strength / detach / pipe.load_lora on the layers it
    memoises (cross_attn.k / v of every block, text_embedding.0 for the merge; cross_attn.o for the fold tables): every forward equals
    the forward with a new cache."""
    import gen_inputs as gi
    from goal_force_amd import lora
    from goal_force_amd.dit import WanModel
    from goal_force_amd.model_fn import ContextCache, model_fn_wan_video
    from goal_force_amd.pipeline import WanVideoPipeline
    cfg = gi.TINY
    dsd = gi.dit_sd(cfg, seed=41)
    model = WanModel(has_image_input=False, require_clip_embedding=False, **cfg)
    model.load_state_dict(dsd, strict=True)
    model = model.to(BF).cuda()
    dev = {k: v.cuda() for k, v in gi.tiny_inputs().items()}
    ts = torch.tensor([995.9], dtype=BF).cuda()

    def fwd(cache):
        return model_fn_wan_video(model, latents=dev["latents"], timestep=ts, context=dev["ctx_posi"], y=dev["y"], context_cache=cache).clone()
    kept = ContextCache()
    base = fwd(kept)
    assert kept.ctx is not None and len(kept.dit_kv) == cfg["num_layers"], "the forward fills the memo"
    assert torch.equal(fwd(kept), base) and torch.equal(fwd(ContextCache()), base)
    names = [f"blocks.{b}.cross_attn.{p}" for b in range(cfg["num_layers"]) for p in "kvo"]
    lsd = _adapter_sd(dsd, names, 8, 306)
    assert lora.attach(model, lsd, alpha=0.7) == len(names)
    att = fwd(kept)
    assert torch.equal(att, fwd(ContextCache())) and not torch.equal(att, base), "the memo outlived lora.attach"
    lora.set_strength(model, 0.0)
    assert torch.equal(fwd(kept), base), "the memo outlived lora.set_strength"
    lora.set_strength(model, 0.7)
    assert torch.equal(fwd(kept), att)
    lora.detach(model)
    assert torch.equal(fwd(kept), base), "the memo outlived lora.detach"
    lsd.update(_adapter_sd(dsd, ["text_embedding.0"], 8, 307))
    assert WanVideoPipeline.from_modules(model).load_lora(model, lsd, alpha=0.7) == len(names) + 1
    merged = fwd(kept)
    assert torch.equal(merged, fwd(ContextCache())) and not torch.equal(merged, base), "the memo outlived pipe.load_lora"


def test_pipeline_call_with_merged_and_attached_adapters():
    """Two steps of the tiny pipeline: an attached adapter changes the result and detaching restores it bit for bit; the merged
    model — caches, patch weight and fold tables included — equals a new model loaded with the merged weights."""
    import gen_inputs as gi
    from goal_force_amd import lora
    from goal_force_amd.dit import WanModel
    from goal_force_amd.pipeline import WanVideoPipeline
    cfg = gi.TINY
    dsd = gi.dit_sd(cfg, seed=41)

    def model(sd):
        m = WanModel(has_image_input=False, require_clip_embedding=False, **cfg)
        m.load_state_dict(sd, strict=True)
        return m.to(BF).cuda()
    pipe = WanVideoPipeline.from_modules(model(dsd))
    dev = {k: v.cuda() for k, v in gi.tiny_inputs().items()}

    def run(p):
        return p.denoise(dev["latents"], dev["ctx_posi"], dev["ctx_nega"], dev["y"], None, num_inference_steps=2, cfg_scale=5.0, controlnet=False).clone()
    plain = run(pipe)
    lsd = _adapter_sd(dsd, LR.GOLDEN_TARGETS, 8, 305, prefix="diffusion_model.")
    in_blocks = {k: v for k, v in lsd.items() if ".blocks." in k}
    n_blocks = len(in_blocks) // 2
    assert lora.attach(pipe.dit, in_blocks, alpha=0.7) == n_blocks == len(LR.GOLDEN_TARGETS) - 2
    att = run(pipe)
    assert bool(torch.isfinite(att).all()) and not torch.equal(att, plain)
    assert lora.detach(pipe.dit) == n_blocks
    assert torch.equal(run(pipe), plain)
    assert pipe.load_lora(pipe.dit, lsd, alpha=0.7) == len(LR.GOLDEN_TARGETS)
    merged = run(pipe)
    fresh = WanVideoPipeline.from_modules(model({k: v.detach().cpu() for k, v in pipe.dit.state_dict().items()}))
    assert torch.equal(merged, run(fresh)) and not torch.equal(merged, plain)


def test_zz_figures():
    """Prints what the gauss comparisons of this run measured (pytest -s)."""
    for k, f in FIG.items():
        print(f"FIG lora {k}: {f['n']} comparisons, worst share of differing bits {f['share']:.3e} (cap {G.SHARE_CAP:.3e}), worst ratio of bar (b) {f['worst']:.3f}")
