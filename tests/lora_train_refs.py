"""The exact chain, an fp32 restatement with faults, and the inputs of the LoRA gradient kernel (goal_force_amd/csrc/gf_lora_grad.hip:
gf_lora_grad), and the fp64 autograd reference of a block with trainable adapters.  Plain helper: CPU tensors in, CPU tensors out, no
GPU and no project import.  The kernel's bars are gemm_refs' two (`judge`) with K = M, the number of tokens summed.

    out[c, j] = bf16( fp32(scale) * sum_{m < M} Y[m, c] T[m, j] )           transposed: the same values stored as out[j, c]

* `grad_chain(Y, T, scale, transposed)` -> gemm_refs.Ref.  The sum in fp64; the scale is ONE fp32 operation followed by the rounding
  to bf16 (lora_refs.rb32: the exact product rounded to fp32, then to bf16 — where the fp32 sum is exact, as in the two exact classes,
  this is the kernel bit for bit).  A zero is +0.  The bars' terms per element: S = |Y|^T |T|, L = |scale| (how far an error of
  the sum travels), m = max(|scale sum|, |out|).  K = M counts the M - 1 additions (inside the slabs and between them) and the
  scale's multiply, each at most one fp32 ulp of a value <= S.
* `slab_plan(M, C)`: the kernel's token split restated — (slabs, rows per slab); slab s is rows s * rows .. min(M, (s + 1) * rows).
  tests/test_lora_grad_gpu.py holds it to gf_lora_grad_slabs / gf_lora_grad_slab_rows on every shape it uses, so the boundaries the
  tests name are the library's.
* `grad_restate(...)`: the same in fp32 torch in the kernel's order — per slab an fp32 partial, summed in ascending tiles of 64
  tokens, the partials added in ascending slab order, then scale and the one rounding — plus GRAD_FAULTS;
  tests/test_lora_grad_refs_cpu.py shows that the restatement passes both bars on every gauss input of the GPU test and that each
  fault is outside one bar or breaks an exact class.
* three data classes (`grad_inputs`): selector and integers are exact (torch.equal), gauss goes through the two bars; gauss outputs
  below gemm_refs.SMALL elements are drawn clear of the rounding boundaries, as gemm_refs.gauss_inputs does.
"""
import math

import torch

import gemm_refs as G
from forward_refs import bits, rb  # noqa: F401
from lora_refs import _gen, f32, rb32

BF = torch.bfloat16
MAX_RANK = 256
COL_TILE, TOKEN_TILE, MIN_TILES, TARGET_WG = 64, 64, 4, 1024
GRAD_FAULTS = ("drop_last_token", "drop_slab", "token_in_two_slabs", "scale_twice", "orientation_ignored", "pad_column_leaks",
               "partial_bf16", "row_2pct")
CLASSES = ("selector", "integers", "gauss")


# ---------------------------------------------------------------------------------------------------------------------
# the token split
def slab_plan(M, C):
    """(slabs, rows per slab): tiles of 64 tokens; enough slabs that column tiles x slabs reaches 1024 workgroups, at most one slab per
    four tiles (rounded up), all equal but the last."""
    ctiles = -(-C // COL_TILE)
    mtiles = -(-M // TOKEN_TILE)
    if mtiles == 0:
        return 0, 0
    target = min(-(-mtiles // MIN_TILES), -(-TARGET_WG // ctiles))
    per = -(-mtiles // target)
    return -(-mtiles // per), per * TOKEN_TILE


def slab_bounds(M, C):
    n, rows = slab_plan(M, C)
    return [(s * rows, min(M, (s + 1) * rows)) for s in range(n)]


def workspace_bytes(M, C, rp):
    return slab_plan(M, C)[0] * -(-C // COL_TILE) * COL_TILE * rp * 4


def smallest_m(C, pred, limit=4096):
    """The smallest M whose slab bounds satisfy pred."""
    for M in range(1, limit):
        if pred(slab_bounds(M, C)):
            return M
    raise RuntimeError("no such M")


def two_slab_m(C):
    return smallest_m(C, lambda b: len(b) == 2)


def one_row_last_slab_m(C):
    return smallest_m(C, lambda b: len(b) >= 3 and b[-1][1] - b[-1][0] == 1)


# ---------------------------------------------------------------------------------------------------------------------
# the chain
def grad_chain(Y, T, scale, transposed=False, acc=None):
    a = f32(scale)
    y64, t64 = Y.double(), T.double()
    if acc is None:
        acc = y64.t() @ t64
    S = y64.abs().t() @ t64.abs()
    v = a * acc
    out = rb32(v) + 0.0                                    # -0 + 0 = +0
    m = torch.maximum(v.abs(), out.abs())
    r = G.Ref(out, m, S, torch.full_like(out, abs(a)), None, None)
    return G.ref_map(r, lambda t: t.t().contiguous()) if transposed else r


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 restatement
def grad_restate(Y, T, scale, transposed=False, bounds=None, tile=TOKEN_TILE, fault=None, rank=None):
    """-> bf16 [C, rp] (transposed: [rp, C]).  bounds: the slabs (None: slab_bounds).  `rank`: the true rank (pad_column_leaks)."""
    M, C = Y.shape
    rp = T.shape[1]
    bounds = slab_bounds(M, C) if bounds is None else list(bounds)
    y, t = Y.float(), T.float().clone()
    one = torch.tensor(f32(scale), dtype=torch.float32)
    if fault == "pad_column_leaks":                        # the columns beyond the true rank are read from somewhere else
        assert rank is not None and rank < rp
        t[:, rank:] = t[:, :1]
    if fault == "drop_last_token" and bounds:
        bounds[-1] = (bounds[-1][0], bounds[-1][1] - 1)
    if fault == "drop_slab":
        bounds = bounds[:-1] if len(bounds) > 1 else []
    if fault == "token_in_two_slabs" and len(bounds) > 1:
        bounds[1] = (bounds[1][0] - 1, bounds[1][1])
    if fault == "token_in_two_slabs" and len(bounds) == 1 and M:
        bounds.append((M - 1, M))
    total = torch.zeros((C, rp))
    for m0, m1 in bounds:
        part = torch.zeros((C, rp))
        for k in range(m0, m1, tile):
            e = min(m1, k + tile)
            part = part + y[k:e].t() @ t[k:e]
        if fault == "partial_bf16":
            part = part.to(BF).float()
        total = total + part
    if fault == "scale_twice":
        total = one * total
    if fault == "row_2pct":
        total[C // 2] *= 1.02
    out = (one * total + 0.0).to(BF)
    if fault == "orientation_ignored":
        return out.view(rp, C) if transposed else out.t().contiguous().view(C, rp)
    return out.t().contiguous() if transposed else out


# ---------------------------------------------------------------------------------------------------------------------
# inputs: dict(Y [M, C], T [M, rp], scale, rank, transposed) with the columns rank .. rp - 1 of T zero; selector also j [M] (the rank
# column of each token), v [M] (its value) and acc (exact)
def _y_exact(shape, g):
    """Multiples of 2^-6 up to 4 in magnitude: every sum of up to 2^11 of them times 2^-1 .. 2^1 is exact in fp32 in any order."""
    return (torch.randint(-256, 257, shape, generator=g).float() / 64).to(BF)


def _orders_agree(d):
    """A gauss draw below gemm_refs.SMALL outputs must give the chain's bits in every order the restatement can state."""
    M, C = d["Y"].shape
    if C * d["T"].shape[1] >= G.SMALL:
        return True
    want = bits(grad_chain(d["Y"], d["T"], d["scale"]).out)
    plans = [slab_bounds(M, C), [(0, M)] if M else []]
    return all(torch.equal(bits(grad_restate(d["Y"], d["T"], d["scale"], bounds=b, tile=tile)), want) for b in plans for tile in (32, 64, 256))


def grad_inputs(cls, M, C, rp, r, scale, transposed=False, seed=0):
    assert rp % 32 == 0 and 1 <= r <= rp <= MAX_RANK and C % 8 == 0
    for attempt in range(512):
        g = _gen(17, CLASSES.index(cls), M, C, rp, r, seed, attempt)
        d = dict(scale=scale, rank=r, transposed=transposed)
        T = torch.zeros((M, rp))
        if cls == "selector":
            j = G.selector_k(M, r) if M else torch.zeros(0, dtype=torch.long)
            v = (torch.randint(0, 2, (M,), generator=g) * 2 - 1).float() * torch.exp2(torch.randint(-1, 2, (M,), generator=g).float())
            T[torch.arange(M), j] = v
            Y = _y_exact((M, C), g)
            acc = torch.zeros((C, rp), dtype=torch.float64)
            acc.index_add_(1, j, (Y.double() * v.double()[:, None]).t().contiguous())
            d.update(Y=Y, T=T.to(BF), j=j, v=v, acc=acc)
        elif cls == "integers":
            Y = torch.randint(-2, 3, (M, C), generator=g).float()
            T[:, :r] = torch.randint(-1, 2, (M, r), generator=g).float()
            if M:
                Y[:, 0] += (torch.arange(M) % 3).float()
                T[:, r - 1] += (torch.arange(M) % 2).float()
            d.update(Y=Y.to(BF), T=T.to(BF))
            assert float((Y.abs().t() @ T.abs()).max()) < 2 ** 24
        else:
            T[:, :r] = torch.randn((M, r), generator=g) / math.sqrt(max(M, 1))
            d.update(Y=torch.randn((M, C), generator=g).to(BF), T=T.to(BF))
            if not _orders_agree(d):
                continue
        return d
    raise RuntimeError(f"grad_inputs({cls}, {M}, {C}, {rp}, {r}): no draw is clear of the rounding boundaries")


def grad_ref(d):
    return grad_chain(d["Y"], d["T"], d["scale"], d["transposed"], acc=d.get("acc"))


# the shapes both test files walk: a covering set — every value of each axis at least once.  The kernel's tiles are 64 columns x 64
# tokens (two MFMA steps of 32), so 31 .. 33 and 63 .. 65 are its edges on the tokens and 56 / 64 / 72 on the columns; 264 and 520 take
# more than one column tile with a ragged last one.  SLAB_C: the column count of the two cases whose M comes from the slab rule.
GRAD_M = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257)
GRAD_C = (8, 56, 64, 72, 264, 520)
GRAD_RANKS = ((32, 1), (64, 4), (256, 33), (32, 4), (64, 33), (256, 1))       # (rank_pad, true rank)
SCALES = (1.0, 0.7, -1.3, 0.0)
SLAB_C = 72


def grad_cases():
    """[(M, C, rank_pad, rank, scale, transposed)]"""
    ms = GRAD_M + (two_slab_m(SLAB_C), one_row_last_slab_m(SLAB_C))
    cases = []
    for i, M in enumerate(ms):
        C = SLAB_C if i >= len(GRAD_M) else GRAD_C[(5 * i + 1) % len(GRAD_C)]
        rp, r = GRAD_RANKS[i % len(GRAD_RANKS)]
        cases.append((M, C, rp, r, SCALES[i % 4], bool(i % 2)))
    # the other orientation and rank of the slab cases, and the widest output on several slabs
    cases.append((ms[-2], 520, 256, 33, 0.7, False))
    cases.append((ms[-1], 264, 32, 4, 1.0, False))
    return cases


# ---------------------------------------------------------------------------------------------------------------------
# a block with trainable adapters: the fp64 autograd reference and the tape's fp32 restatement
#
# `adapters`: {layer: [(down_pad [rank_pad, in] bf16, up_pad [out, rank_pad] bf16, scaling)]} in attach order, layer one of LAYERS.
# Gradient names: "<layer>.lora_A.<i>" / "<layer>.lora_B.<i>" (i the position on the layer) beside tape_refs' 27 names and "dx".
#
# * `adapted_grads_ref`: tape_refs.block_grads_ref's fp64 block with each adapted weight replaced by W + sum_i s_i B_i A_i on fp64
#   leaves A_i, B_i — exact algebra for peft's unmerged forward y + s (x A^T) B^T.  The padding's gradients are identically zero
#   there (its rows of t and dt are), and tape_refs.row_stat then asks the device for exact zeros.
# * `adapted_block_chain`: tape_refs.block_chain with the adapters' launches restated where DiTBlockFn runs them.  tape_refs' stages
#   are reached through its module-level names, so the restatement swaps four of them for the duration of one call (`_lin`, `_gemm`
#   for the cross-attention's o + residual, `linear_dw`, `linear_dx`) and leaves them as they were: forward  y = up_chain(gemm(x, W,
#   b), t = gemm(x, A), B, s) per adapter (lora_refs.restate, the last one with the layer's epilogue); backward per adapter
#   t = gemm(x, A), dt = gemm(dy, B^T), dB = grad_restate(dy, t, s), dA = grad_restate(x, dt, s, transposed),
#   dx = restate(dx, dt, A^T, s).  block_bwd calls linear_dw once per Linear in BWD_ORDER, which is how a call is told its layer.
# * the row statistic is tape_refs' (ratio of the device's distance from fp64 over the order-0 restatement's, per row and column);
#   the adapters' tensors form two groups of their own and dx behind adapters a third.  LORA_ROW_WORST: the worst ratio of the
#   order-1 restatement over block_cases(), measured by tests/test_lora_train_cpu.py::test_lora_row_worst_reproduces; the device's
#   bar is 1.25 x that (tape_refs.ROW_BAR's rule).
import contextlib  # noqa: E402

import lora_refs as LR  # noqa: E402
import tape_refs as TP  # noqa: E402

LAYERS = tuple(f"{a}.{p}" for a in ("self_attn", "cross_attn") for p in "qkvo") + ("ffn.0", "ffn.2")
BWD_ORDER = ("ffn.2", "ffn.0", "cross_attn.o", "cross_attn.q", "cross_attn.k", "cross_attn.v", "self_attn.o", "self_attn.q", "self_attn.k",
             "self_attn.v")
# measured: 7.617 (lora_up), 6.483 (lora_down), 1.345 (dx_lora); both adapter figures come from the rank-4 cases with 7 context rows,
# where a row of dB / dA on cross_attn.k / v is ONE sum over seven tokens (tape_refs' attn_weight group, more so: 4 live columns)
LORA_ROW_WORST = {"lora_up": 7.62, "lora_down": 6.49, "dx_lora": 1.35}


def lora_bars():
    return {**TP.ROW_BAR, **{k: 1.25 * v for k, v in LORA_ROW_WORST.items()}}


def lora_group(name, adapted_dx=True):
    if ".lora_B." in name:
        return "lora_up"
    if ".lora_A." in name:
        return "lora_down"
    if name == "dx" and adapted_dx:
        return "dx_lora"
    return TP.group(name)


def lora_failures(stats, bars=None):
    bars = lora_bars() if bars is None else bars
    out = []
    for n, s in stats.items():
        bar = bars[lora_group(n)]
        if not s["worst"] <= bar:
            out.append(f"{n}: {s['where']} is {s['worst']:.3f} x the restatement's distance from fp64 (bar {bar:.3f}, group {lora_group(n)})")
        if s["zero_bad"]:
            out.append(f"{n}: {s['zero_bad']} slice(s) whose reference is identically zero are not exactly zero")
    return out


def lora_worst_by_group(stats):
    out = {}
    for n, s in stats.items():
        out[lora_group(n)] = max(out.get(lora_group(n), 0.0), s["worst"])
    return out


def block_cases():
    """tape_refs' block cases at 64 / 65 / 130 tokens with 64 / 65 / 7 context rows, q pre-scale on, and the 72-token pair with it on and
    off — each with (rank, scaling, init) per adapter set: rank 4 at scaling 1, rank 33 at 0.7 (Gaussian lora_B), and peft's init."""
    by = {c["name"]: c for c in TP.cases()}
    sets = {"r4": (4, 1.0, "gauss"), "r33": (33, 0.7, "gauss"), "peft": (4, 1.0, "peft")}
    pick = [("tiny-64-64", "r4"), ("tiny-65-65", "r33"), ("tiny-130-7", "r4"), ("tiny-72-7", "r33"), ("tiny-72-7-plainq", "r4"), ("tiny-64-64", "peft")]
    return [dict(by[c], name=f"{c}-{a}", rank=sets[a][0], scaling=sets[a][1], init=sets[a][2]) for c, a in pick]


def make_adapters(sd, rank, scaling, init="gauss", seed=0, layers=LAYERS, second=None):
    """Adapters for `layers` of a block state dict: lora_A ~ U(-1/sqrt(in), 1/sqrt(in)), lora_B ~ N(0, 1/r) (init "peft": zero), both bf16
    and zero-padded to a multiple of 32.  `second`: (rank, scaling) of a second adapter on self_attn.q and ffn.2."""
    out = {}
    for li, layer in enumerate(layers):
        n_out, k_in = sd[layer + ".weight"].shape
        specs = [(rank, scaling)] + ([second] if second and layer in ("self_attn.q", "ffn.2") else [])
        for ai, (r, s) in enumerate(specs):
            g = _gen(23, seed, li, ai, r)
            rp = -(-r // 32) * 32
            down, up = torch.zeros((rp, k_in)), torch.zeros((n_out, rp))
            down[:r] = (torch.rand((r, k_in), generator=g) * 2 - 1) / math.sqrt(k_in)
            if init != "peft":
                up[:, :r] = torch.randn((n_out, r), generator=g) / math.sqrt(r)
            out.setdefault(layer, []).append((down.to(BF), up.to(BF), s))
    return out


def adapted_grads_ref(cfg, sd, adapters, x, ctx, t_mod, dout, grid):
    """(dx, {name: gradient}) in fp64; the base weights' gradients are those of W_eff (= dL/dW: W enters only through W_eff)."""
    from oracle import wan_oracle as wo
    with torch.enable_grad():
        leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        lo = {}
        eff = dict(leaves)
        for layer, ads in adapters.items():
            w = leaves[layer + ".weight"]
            for i, (down, up, s) in enumerate(ads):
                a, b = down.double().requires_grad_(True), up.double().requires_grad_(True)
                lo[f"{layer}.lora_A.{i}"], lo[f"{layer}.lora_B.{i}"] = a, b
                w = w + f32(s) * (b @ a)
            eff[layer + ".weight"] = w
        xd = x.double()[None].requires_grad_(True)
        fr = wo.rope_freqs_3d(cfg["dim"] // cfg["num_heads"], *grid)
        y = wo.dit_block(xd, ctx.double()[None], t_mod.double(), fr, eff, "", cfg["num_heads"], cfg["eps"])
        y.backward(dout.double()[None])
    grads = {k: v.grad for k, v in leaves.items()}
    grads.update({k: v.grad for k, v in lo.items()})
    return xd.grad[0], grads


@contextlib.contextmanager
def _adapted_stages(sd, adapters, out):
    """tape_refs' four stage names with the adapters' launches added, for one block_chain call; `out` collects the adapters' gradients."""
    orig = dict(_lin=TP._lin, _gemm=TP._gemm, linear_dw=TP.linear_dw, linear_dx=TP.linear_dx)
    calls = [0]

    def up_all(y, xin, layer, order, epi=G.EPI_BIAS, resid=None):
        ads = adapters.get(layer, ())
        for i, (down, up, s) in enumerate(ads):
            last = i + 1 == len(ads)
            y = LR.restate(y, orig["_gemm"](xin, down, None, order), up, s, epi if last else G.EPI_BIAS, resid if last else None)
        return y

    def _lin(xin, sd_, pre, order):
        return up_all(orig["_gemm"](xin, sd_[pre + ".weight"], sd_[pre + ".bias"], order), xin, pre, order)

    def _gemm(a, w, bias, order, epi=G.EPI_BIAS, resid=None):
        if epi == G.EPI_RESID and w is sd["cross_attn.o.weight"] and adapters.get("cross_attn.o"):
            return up_all(orig["_gemm"](a, w, bias, order), a, "cross_attn.o", order, epi, resid)
        return orig["_gemm"](a, w, bias, order, epi, resid)

    def linear_dw(dy, xin, order=0, fault=None):
        layer = BWD_ORDER[calls[0] % len(BWD_ORDER)]
        calls[0] += 1
        for i, (down, up, s) in enumerate(adapters.get(layer, ())):
            t = orig["_gemm"](xin, down, None, order)
            dt = orig["_gemm"](dy, up.t().contiguous(), None, order)
            tile = TOKEN_TILE if order == 0 else TOKEN_TILE // 2
            out[f"{layer}.lora_B.{i}"] = grad_restate(dy, t, s, tile=tile)
            out[f"{layer}.lora_A.{i}"] = grad_restate(xin, dt, s, transposed=True, tile=tile)
        return orig["linear_dw"](dy, xin, order, fault)

    def linear_dx(dy, w, order=0):
        dx = orig["linear_dx"](dy, w, order)
        layer = next(n for n in LAYERS if sd[n + ".weight"] is w)
        for down, up, s in adapters.get(layer, ()):
            dt = orig["_gemm"](dy, up.t().contiguous(), None, order)
            dx = LR.restate(dx, dt, down.t().contiguous(), s)
        return dx

    TP._lin, TP._gemm, TP.linear_dw, TP.linear_dx = _lin, _gemm, linear_dw, linear_dx
    try:
        yield
    finally:
        TP._lin, TP._gemm, TP.linear_dw, TP.linear_dx = orig["_lin"], orig["_gemm"], orig["linear_dw"], orig["linear_dx"]


def adapted_block_chain(cfg, sd, adapters, x, ctx, t_mod, dout, grid, order=0, prescale=True):
    """(dx bf16, {name: gradient bf16}, the block's output bf16) of the tape with the adapters, restated."""
    lo = {}
    with _adapted_stages(sd, adapters, lo):
        s = TP.block_fwd(cfg, sd, x, ctx, t_mod, grid, order, prescale)
        dx, g = TP.block_bwd(s, dout)
    g.update(lo)
    return dx, g, s.out


# ---------------------------------------------------------------------------------------------------------------------
# the training loop on the tiny expert (tests/golden/make_lora_train_golden.py -> tests/golden/g22_lora_train.npz)
LOOP = dict(rank=4, learning_rate=1e-3, weight_decay=1e-2, max_grad_norm=1.0, steps=4, timestep_ids=(137, 300, 50, 600),
            targets="q,k,v,o,ffn.0,ffn.2")


def loop_adapters(cfg, dit_sd):
    """{linear name: (lora_A [r, in], lora_B [out, r])} bf16 of the loop's start: every block Linear of the tiny expert, lora_A in
    peft's range, lora_B at 0.05 N(0, 1) (from zero the first steps would move lora_B alone)."""
    out = {}
    r = LOOP["rank"]
    for b in range(cfg["num_layers"]):
        for li, layer in enumerate(LAYERS):
            name = f"blocks.{b}.{layer}"
            n_out, k_in = dit_sd[name + ".weight"].shape
            g = _gen(29, b, li)
            a = ((torch.rand((r, k_in), generator=g) * 2 - 1) / math.sqrt(k_in)).to(BF)
            out[name] = (a, (0.05 * torch.randn((n_out, r), generator=g)).to(BF))
    return out
