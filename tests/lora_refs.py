"""The exact chain, an fp32 restatement with faults, and the inputs of the LoRA kernels (goal_force_amd/csrc/gf_lora.hip: gf_lora_merge,
gf_lora_up).  Plain helper: CPU tensors in, CPU tensors out, no GPU and no project import.  The bars are gemm_refs' two (`judge`).

Both kernels are Y[r, c] <- epi(bf16(Y + bf16(fp32(scale) * bf16(sum_j R[r, j] Ct[c, j])))):
    gf_lora_merge   Y = W [n_out, k_in],  R = up [n_out, rank],   Ct = down^T,          scale = alpha, no epilogue
    gf_lora_up      Y = y0 [M, N],        R = t [M, rank_pad],    Ct = up [N, rank_pad], the six gf_epilogue forms on y
so one chain and one restatement serve both (`merge_*` and `up_*` are the two spellings of the operands).

* `chain(y0, rf, cf, scale, epi, resid, gate)` -> gemm_refs.Ref.  The sum in fp64; every later operation is ONE fp32 operation
  followed by the rounding to bf16, which is what torch's bf16 kernels (the reference's loader, peft's forward) and the kernel do:
  `rb32(v)` rounds the exact fp64 value to fp32 first (a product of a 24-bit and an 8-bit significand, or a sum of two bf16 values far
  apart, is not always an fp32 number) and then to bf16.  scale is fp32(scale), not the double.
      d = bf16(acc)      s = bf16(fp32(scale) d)      y = bf16(y0 + s)      out = epi(y, resid, gate) as gemm_refs.chain states it
  The bars' terms, per element:
      S = |R| |Ct|^T;   L = L_epi |scale|  (how far an error of the accumulator travels: through the scale, then the epilogue's slope);
      m = m_epi(y) + L_epi (|scale| |d| + |s|): gemm_refs.chain's m for the epilogue on y (the stages after y, each rounded again),
          raised by what a flipped rounding BEFORE y costs — a step of d (<= 2^-7 |d|) reaches s through |scale| and s is rounded
          again (one more step of s), y is rounded again (its own step is inside m_epi), and all of it passes the epilogue's slope.
          Neither |acc| nor |d| enters m on its own: at scale 0 the output must be epi(y0) exactly.
* `restate(...)`: the same in fp32 torch with the sum in the header's stated order — the rank in chunks of 32 (zero-padded), ascending,
  each chunk one fp32 matrix product added to the accumulator — plus the FAULTS; tests/test_lora_cpu.py shows that the restatement
  passes both bars on every gauss input of the GPU test and that each fault does not.
* three data classes per kernel (`merge_inputs`, `up_inputs`): selector, integers (both exact: torch.equal), gauss (the two bars; small
  outputs are drawn clear of the rounding boundaries as gemm_refs.gauss_inputs does).
"""
import math

import numpy as np
import torch

import gemm_refs as G
from forward_refs import bits, rb  # noqa: F401

BF = torch.bfloat16
MAX_RANK = 256
FAULTS = ("drop_last_rank", "neighbour_row", "down_transposed", "alpha_bf16", "alpha_first", "no_first_rounding", "add_before_scale")
UP_FAULTS = ("t_unrounded", "epi_on_y0", "gate_after_resid")
HAS_R = (G.EPI_GATE_RESID, G.EPI_RESID, G.EPI_MUL)


def f32(x):
    """fp32(x) as a Python float."""
    return float(np.float32(x))


def rb32(v):
    """One fp32 operation's result rounded to bf16: the exact value (fp64) -> fp32 -> bf16, returned as fp64."""
    return v.float().to(BF).double()


# ---------------------------------------------------------------------------------------------------------------------
# the chain
def chain(y0, rf, cf, scale, epi=G.EPI_BIAS, resid=None, gate=None, acc=None):
    a = f32(scale)
    rf64, cf64 = rf.double(), cf.double()
    if acc is None:
        acc = rf64 @ cf64.t()
    S = rf64.abs() @ cf64.abs().t()
    d = rb(acc)
    s = rb32(a * d)
    y = rb32(y0.double() + s)
    _, m_e, _, L_e = G.chain(y, None, epi, resid, gate)
    r64 = None if resid is None else resid.double()
    if epi in (G.EPI_GELU, G.EPI_SILU):
        out = G.chain(y, None, epi, None, None)[0]
    elif epi == G.EPI_GATE_RESID:
        out = rb32(r64 + rb32(gate.double() * y))
    elif epi == G.EPI_RESID:
        out = rb32(r64 + y)
    elif epi == G.EPI_MUL:
        out = rb32(y * r64)
    else:
        out = y
    m = m_e + L_e * (abs(a) * d.abs() + s.abs())
    return G.Ref(out, m, S, L_e * abs(a), None, None), y


def merge_chain(d):
    """Ref of a merge input dict: the reference's W + alpha * mm(up, down) in bf16."""
    return chain(d["w"], d["up"], d["down"].t(), d["alpha"], acc=d.get("acc"))[0]


def up_chain(d, epi):
    """(Ref, the exact y) of an up input dict under one epilogue."""
    return chain(d["y0"], d["t"], d["up"], d["scale"], epi, d["resid"] if epi in HAS_R else None,
                 d["gate"] if epi == G.EPI_GATE_RESID else None, acc=d.get("acc"))


# ---------------------------------------------------------------------------------------------------------------------
# the fp32 restatement
def sum_f32(rf, cf, chunk=32, reverse=False):
    """R Ct^T in fp32: the rank zero-padded to a multiple of `chunk`, one product per chunk, ascending (or descending)."""
    r = rf.shape[1]
    rp = -(-r // chunk) * chunk
    a = torch.zeros((rf.shape[0], rp))
    b = torch.zeros((cf.shape[0], rp))
    a[:, :r], b[:, :r] = rf.float(), cf.float()
    acc = torch.zeros((rf.shape[0], cf.shape[0]))
    order = range(0, rp, chunk)
    for c in (reversed(order) if reverse else order):
        acc = acc + a[:, c:c + chunk] @ b[:, c:c + chunk].t()
    return acc


def restate(y0, rf, cf, scale, epi=G.EPI_BIAS, resid=None, gate=None, chunk=32, reverse=False, fault=None, x=None, down=None):
    """-> bf16.  `fault`: one of FAULTS (both kernels) or UP_FAULTS (the attached form; t_unrounded needs x and down, the operands
    t = bf16(x down^T) was made from)."""
    f = lambda t: t.float()          # noqa: E731
    one = torch.tensor(f32(scale), dtype=torch.float32)
    rf, cf = f(rf).clone(), f(cf).clone()
    if fault == "t_unrounded":
        rf = sum_f32(x, down, 64)                                  # x down^T left in fp32
    if fault == "drop_last_rank":
        live = int(torch.nonzero((rf != 0).any(0) & (cf != 0).any(0)).max()) + 1      # the true rank inside the padding
        rf, cf = rf[:, :live - 1], cf[:, :live - 1]
    if fault == "neighbour_row":                                   # one row of Y takes the row factor of the row after it
        r = rf.shape[0] // 2
        rf[r] = rf[(r + 1) % rf.shape[0]]
    if fault == "down_transposed":                                 # the column factor's memory indexed [j][c] where it is [c][j]
        cf = cf.contiguous().view(cf.shape[1], cf.shape[0]).t()
    if fault == "alpha_bf16":
        one = one.to(BF).float()
    if fault == "alpha_first":                                     # the scale goes into the operand: the products are no longer exact
        rf, one = rf * one, torch.tensor(1.0)
    acc = sum_f32(rf, cf, chunk, reverse)
    d = acc if fault == "no_first_rounding" else rb(acc)
    yy = f(y0)
    if fault == "epi_on_y0":
        s = rb(one * d)
        return (_epi_f32(yy, epi, resid, gate, None).to(BF).float() + s).to(BF)
    if fault == "add_before_scale":
        y = rb(one * rb(yy + d))
    else:
        y = rb(yy + rb(one * d))
    return _epi_f32(y, epi, resid, gate, fault).to(BF)


def _epi_f32(y, epi, resid, gate, fault):
    f = lambda t: t.float()          # noqa: E731
    if epi in (G.EPI_GELU, G.EPI_SILU):
        return G._act_f32(y, epi)
    if epi == G.EPI_GATE_RESID:
        return f(gate) * rb(f(resid) + y) if fault == "gate_after_resid" else f(resid) + rb(f(gate) * y)
    if epi == G.EPI_RESID:
        return f(resid) + y
    if epi == G.EPI_MUL:
        return y * f(resid)
    return y


def merge_restate(d, **kw):
    return restate(d["w"], d["up"], d["down"].t(), d["alpha"], **kw)


def up_restate(d, epi, **kw):
    return restate(d["y0"], d["t"], d["up"], d["scale"], epi, d["resid"], d["gate"], x=d.get("x"), down=d.get("down"), **kw)


# ---------------------------------------------------------------------------------------------------------------------
# inputs.  merge: dict(w [n, k], up [n, r], down [r, k], alpha);  up: dict(y0 [M, N], t [M, rp], up [N, rp], resid [M, N], gate [N],
# scale, rank) with columns rank .. rp - 1 of t and up zero.  selector dicts carry j (the rank column per row) and acc (exact).
def _gen(*key):
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v)) % (2 ** 61 - 1)
    return torch.Generator().manual_seed(seed)


def _pow2_signed(n, g):
    return (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float() * torch.exp2(torch.randint(-1, 2, (n,), generator=g).float())


def _selector(rows, rank, rp, g):
    """Row factor [rows, rp]: row i is one +-2^k (k in -1..1) at rank column j(i) < rank — every rank column taken when rows >= rank."""
    j = G.selector_k(rows, rank)
    rf = torch.zeros((rows, rp))
    v = _pow2_signed(rows, g)
    rf[torch.arange(rows), j] = v
    return rf.to(BF), j, v.double()


def _small_ok(d, chain_of, restate_of, numel):
    """A gauss draw below gemm_refs.SMALL outputs must give the chain's bits in every order the restatement can state."""
    if numel >= G.SMALL:
        return True
    want = bits(chain_of(d))
    return all(torch.equal(bits(restate_of(d, chunk=c, reverse=rev)), want) for c in (8, 32, 256) for rev in (False, True))


def merge_inputs(cls, n, k, r, alpha, seed=0):
    for attempt in range(256):
        g = _gen(11, ("selector", "integers", "gauss").index(cls), n, k, r, seed, attempt)
        d = dict(alpha=alpha, rank=r)
        if cls == "selector":
            up, j, v = _selector(n, r, r, g)
            down, w = G._band_bf16((r, k), g), G._band_bf16((n, k), g)
            d.update(up=up, down=down, w=w, j=j, acc=v[:, None] * down.double()[j])
        elif cls == "integers":
            up = torch.randint(-2, 3, (n, r), generator=g).float()
            down = torch.randint(-1, 2, (r, k), generator=g).float()
            up[:, 0] += (torch.arange(n) % 3).float()
            down[r - 1] += (torch.arange(k) % 2).float()
            w = torch.randint(-4, 5, (n, k), generator=g).float()
            d.update(up=up.to(BF), down=down.to(BF), w=w.to(BF))
            acc = up.double() @ down.double()
            assert float(acc.abs().max()) <= 256 and torch.equal(rb(acc), acc), "integer class: the sum is not exactly representable"
        else:
            d.update(up=torch.randn((n, r), generator=g).to(BF), down=(torch.randn((r, k), generator=g) / math.sqrt(r)).to(BF),
                     w=torch.randn((n, k), generator=g).to(BF))
            if not _small_ok(d, lambda x: merge_chain(x).out, merge_restate, n * k):
                continue
        return d
    raise RuntimeError(f"merge_inputs({cls}, {n}, {k}, {r}): no draw is clear of the rounding boundaries")


def up_inputs(cls, M, N, rp, r, scale, seed=0, K=64):
    """gauss also carries x [M, K] and down [rp, K] with t = bf16(x down^T) (the fp64 product, rounded once)."""
    assert rp % 32 == 0 and 1 <= r <= rp <= MAX_RANK
    for attempt in range(256):
        g = _gen(13, ("selector", "integers", "gauss").index(cls), M, N, rp, r, seed, attempt)
        d = dict(scale=scale, rank=r)
        up = torch.zeros((N, rp))
        if cls == "selector":
            t, j, v = _selector(M, r, rp, g)
            up = up.to(BF)
            up[:, :r] = G._band_bf16((N, r), g)
            d.update(t=t, up=up, y0=G._band_bf16((M, N), g), resid=G._band_bf16((M, N), g), gate=G._band_bf16((N,), g), j=j,
                     acc=v[:, None] * up.double()[:, j].t())
        elif cls == "integers":
            t = torch.zeros((M, rp))
            t[:, :r] = torch.randint(-2, 3, (M, r), generator=g).float()
            up[:, :r] = torch.randint(-1, 2, (N, r), generator=g).float()
            t[:, 0] += (torch.arange(M) % 3).float()
            up[:, r - 1] += (torch.arange(N) % 2).float()
            d.update(t=t.to(BF), up=up.to(BF), y0=torch.randint(-4, 5, (M, N), generator=g).float().to(BF),
                     resid=torch.randint(-2, 3, (M, N), generator=g).float().to(BF),
                     gate=(torch.randint(0, 2, (N,), generator=g) * 2 - 1).float().to(BF))
            acc = t.double() @ up.double().t()
            assert float(acc.abs().max()) <= 256 and torch.equal(rb(acc), acc), "integer class: the sum is not exactly representable"
        else:
            x = torch.randn((M, K), generator=g).to(BF)
            down = torch.zeros((rp, K))
            down[:r] = torch.randn((r, K), generator=g) / math.sqrt(K)
            down = down.to(BF)
            up[:, :r] = torch.randn((N, r), generator=g) / math.sqrt(r)
            d.update(x=x, down=down, t=rb(x.double() @ down.double().t()).to(BF), up=up.to(BF),
                     y0=torch.randn((M, N), generator=g).to(BF), resid=torch.randn((M, N), generator=g).to(BF),
                     gate=torch.randn((N,), generator=g).to(BF))
            if not all(_small_ok(d, lambda x_, e=e: up_chain(x_, e)[0].out, lambda x_, e=e, **kw: up_restate(x_, e, **kw), M * N)
                       for e in G.EPIS):
                continue
        return d
    raise RuntimeError(f"up_inputs({cls}, {M}, {N}, {rp}, {r}): no draw is clear of the rounding boundaries")


# ---------------------------------------------------------------------------------------------------------------------
# the shapes both test files walk: covering sets — every value of each axis at least once.  The kernels' tile is 64 x 64 (rows x
# columns), so 63 / 64 / 65 on either axis are its edges; k_in and N are multiples of 8.
MERGE_N = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513)
MERGE_K = (8, 24, 64, 72, 128, 136, 256, 264, 520, 56)
MERGE_R = (1, 4, 8, 31, 32, 33, 64, 96, 128, 255, 256)
ALPHAS = (1.0, 0.7, -1.3, 0.0)
MERGE_CASES = [(MERGE_N[i], MERGE_K[(3 * i) % len(MERGE_K)], MERGE_R[(7 * i + 2) % len(MERGE_R)], ALPHAS[i % 4]) for i in range(11)] + \
              [(129, 520, 256, 0.7), (64, 56, 33, -1.3), (65, 8, 255, 1.0), (127, 24, 1, 0.7), (128, 128, 128, -1.3), (17, 136, 64, 0.0),
               (513, 264, 4, -1.3), (1, 256, 96, 0.7), (63, 72, 32, 0.0)]
UP_M = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 513, 63, 64, 65)
UP_N = (8, 64, 72, 136, 256, 264, 520, 56)
UP_RANKS = ((32, 1), (64, 33), (128, 128), (256, 255), (32, 32), (64, 64), (256, 256))       # (rank_pad, true rank)
SCALES = (1.0, 0.7, 0.0)
UP_CASES = [(UP_M[i], UP_N[(3 * i + 1) % len(UP_N)], *UP_RANKS[i % len(UP_RANKS)], SCALES[i % 3]) for i in range(len(UP_M))] + \
           [(513, 520, 256, 255, 0.7), (130, 56, 32, 1, 0.7)]


# ---------------------------------------------------------------------------------------------------------------------
# module level: the fp64 statements the GPU module tests and the golden compare with
def merged_weight(w, up, down, alpha):
    """bf16 [out, in]: the chain on one Linear's weight (its three roundings alone, without the bars' terms)."""
    d = rb(up.double() @ down.double())
    return rb32(w.double() + rb32(f32(alpha) * d)).to(BF)


def merged_state(sd, lora_sd, names, alpha):
    """The state dict after GeneralLoRALoader.load by the chain: `names` = {module name: (lora_B key, lora_A key)} of the matched modules."""
    out = dict(sd)
    for name, (kb, ka) in names.items():
        out[name + ".weight"] = merged_weight(sd[name + ".weight"], lora_sd[kb].to(BF), lora_sd[ka].to(BF), alpha)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# g21: the reference's loader on the tiny expert of g5 (tests/golden/make_lora_golden.py).  Everything below is seeded: the generator
# and the tests build the same base weights and adapter files, the fixture holds what the reference made of them.
GOLDEN_TARGETS = tuple(f"blocks.0.{a}.{p}" for a in ("self_attn", "cross_attn") for p in "qkvo") + \
    ("blocks.0.ffn.0", "blocks.0.ffn.2", "blocks.1.self_attn.q", "blocks.1.ffn.2", "text_embedding.0", "head.head")
# (spelling of the lora_B key, prefix, rank, alpha); the second load stacks on the first
GOLDEN_LOADS = (("lora_B.weight", "diffusion_model.", 4, 1.0), ("lora_B.default.weight", "", 33, 0.7))
GOLDEN_CLASSES = ("integers", "gauss")
# keys that match no module (a block the model does not have, a name that is none, the kohya spelling) and keys the rule skips
GOLDEN_STRAYS = ("blocks.9.self_attn.q.lora_B.weight", "blocks.0.self_attn.qq.lora_B.weight", "diffusion_model.nothing.here.lora_B.default.weight",
                 "lora_unet_blocks_0_self_attn_q.lora_up.weight", "lora_unet_blocks_0_self_attn_q.lora_down.weight",
                 "lora_unet_blocks_0_self_attn_q.alpha", "blocks.0.self_attn.q.diff_b")


def golden_base_sd(cls):
    """The tiny expert's state dict (gen_inputs.dit_sd(TINY, 41), bf16); class integers: the targeted weights are small integers."""
    import gen_inputs as gi
    sd = gi.dit_sd(gi.TINY, seed=41)
    if cls == "integers":
        g = _gen(21, 0)
        for name in GOLDEN_TARGETS:
            w = sd[name + ".weight"]
            sd[name + ".weight"] = torch.randint(-4, 5, tuple(w.shape), generator=g).float().to(BF)
    return sd


def golden_lora_sd(load, cls, base_sd):
    """The adapter file of GOLDEN_LOADS[load] in one data class: bf16 lora_A / lora_B pairs for GOLDEN_TARGETS, plus GOLDEN_STRAYS."""
    spelling, prefix, r, _ = GOLDEN_LOADS[load]
    g = _gen(21, 1 + load, GOLDEN_CLASSES.index(cls))
    sd = {}
    for name in GOLDEN_TARGETS:
        n, k = base_sd[name + ".weight"].shape
        if cls == "integers":
            up = torch.randint(-2, 3, (n, r), generator=g).float()
            down = torch.randint(-1, 2, (r, k), generator=g).float()
        else:
            up = torch.randn((n, r), generator=g) / math.sqrt(k)
            down = torch.randn((r, k), generator=g) / math.sqrt(r)
        kb = f"{prefix}{name}.{spelling}"
        sd[kb.replace(".lora_B.", ".lora_A.")] = down.to(BF)
        sd[kb] = up.to(BF)
    for key in GOLDEN_STRAYS:
        sd[key] = torch.ones((2, 2), dtype=BF)
    for key in [k for k in GOLDEN_STRAYS if ".lora_B." in k]:
        sd[key.replace(".lora_B.", ".lora_A.")] = torch.ones((2, 2), dtype=BF)
    return sd


def sha(t):
    """sha256 of a bf16 tensor's bits."""
    import hashlib
    return hashlib.sha256(bits(t).numpy().tobytes()).hexdigest()


def golden_reference_weights(g21, cls):
    """[{module name: the REFERENCE's merged bf16 weight} after load 0, ... after load 1] rebuilt from the fixture: the chain on the
    seeded inputs, with the elements the fixture lists (where the reference's own bf16 arithmetic differs from the chain) set to
    the reference's values — and proven to be the reference's tensor bit for bit by the sha256 the fixture holds of it.
    -> (the list, [the chain's own weights per load], [the name dicts per load])."""
    import json
    base = golden_base_sd(cls)
    refs, chains, dicts = [], [], []
    for load, (_, _, _, alpha) in enumerate(GOLDEN_LOADS):
        lsd = golden_lora_sd(load, cls, base)
        names = {k: tuple(v) for k, v in json.loads(str(g21[f"name_dict_{load}"])).items()}
        hit = {n: names[n] for n in GOLDEN_TARGETS}
        ch = merged_state(base, lsd, hit, alpha)
        ref = {}
        for i, n in enumerate(GOLDEN_TARGETS):
            w = ch[n + ".weight"].clone()
            idx = torch.from_numpy(g21[f"{cls}_{load}_{i}_idx"].astype(np.int64))
            val = torch.from_numpy(g21[f"{cls}_{load}_{i}_val"].astype(np.int16)).view(BF)
            w.view(-1)[idx] = val
            assert sha(w) == str(g21[f"{cls}_{load}_{i}_sha"]), f"g21 {cls} load {load} {n}: the rebuilt tensor is not the reference's"
            ref[n] = w
        refs.append(ref)
        chains.append({n: ch[n + ".weight"] for n in GOLDEN_TARGETS})
        dicts.append(names)
        base = dict(base)
        for n in GOLDEN_TARGETS:                # the second load stacks on what the REFERENCE left
            base[n + ".weight"] = ref[n]
    return refs, chains, dicts
