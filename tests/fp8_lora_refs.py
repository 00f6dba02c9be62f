"""What tests/test_fp8_lora_cpu.py and tests/test_fp8_lora_gpu.py share: the shapes of the gf_gemm_fp8_lora kernel tests, the Python
restatement of gf_gemm_fp8_lora_ok, the operand classes and the fp64 chain of the header's formula

    y0       = bf16( (A8 · W8^T)[m,n] * row_scale[m] + bias[n] )
    out[m,n] = epi( bf16( y0 + bf16( scale * bf16( sum_j t[m,j] * up[n,j] ) ) ), resid, gate )

built from the two chains the suite already has: gemm_refs.chain (y0) and lora_refs.chain (the adapter and the epilogue).

The `integers` class is exact at every step of that formula (small integers as e4m3 codes, power-of-two row scales, integer bias /
t / up / resid / gate: every fp32 operation of the kernel is exact up to the bf16 roundings the formula names), so the device must
equal the fp64 chain bit for bit under the four epilogues whose arithmetic is elementary (bias, gate_resid, resid, mul); the two
activations are held by the equality with the two-launch pair, whose own epilogue tests/test_lora_gpu.py pins.  The `gauss` class comes
from the project's quantisers on the device and is compared with the pair only: same operands, same k slots, same roundings."""
import itertools

import torch

import gemm_refs as G
import lora_refs as LR

BF = torch.bfloat16
RANK_PADS = (32, 64)                       # the fused range
FUSED_MIN_M = 512
# the 4-wave kernel's floor, ragged rows inside a wave and across the 128-row wave boundary, a ragged tile group
MS = (512, 513, 640, 767, 769, 2305)
# one store piece, the wn boundary, a second column tile holding one piece
NS = (8, 120, 128, 136, 256, 264, 520)
KS = (128, 256, 640)                       # 1, 2 and 5 K tiles
RANKS = ((32, 1), (32, 4), (64, 33), (64, 64))      # (rank_pad, true rank)
SCALES = (1.0, 0.7, -1.3, 0.0)
EXACT_EPIS = (G.EPI_BIAS, G.EPI_GATE_RESID, G.EPI_RESID, G.EPI_MUL)
# Shapes: every M with every K (18), the N values walked with a stride coprime to both (each occurs at least twice, and with different M
# and K).  At EACH shape the GPU test runs all four ranks x all four scales x all six epilogues on gauss operands against the pair;
# the two exact classes, whose fp64 chain is built on the host, take one (rank, scale) per shape — EXACT_AT walks the sixteen pairs
# with a stride of 5 (coprime to 16, to 6 and to 3), so over the 18 shapes every rank meets every scale, M and K residue.
SHAPES = [(MS[i % len(MS)], NS[(5 * i + 1) % len(NS)], KS[i // len(MS)]) for i in range(len(MS) * len(KS))]
EXACT_AT = [(RANKS[(5 * i) % 16 // 4], SCALES[(5 * i) % 16 % 4]) for i in range(len(SHAPES))]
CASES = [(M, N, K, *EXACT_AT[i][0], EXACT_AT[i][1]) for i, (M, N, K) in enumerate(SHAPES)]       # the exact classes' cases


def ok_py(M, N, K, rank_pad, prefer_8wave=0):
    """gf_gemm_fp8_lora_ok restated: the 4-wave fp8 dispatch conditions on dense rows, the fused ranks, prefer_8wave off."""
    if prefer_8wave:
        return 0
    if M < FUSED_MIN_M or M >= 2 ** 30 or N <= 0 or N >= 2 ** 30 or N % 8 or K <= 0 or K % 128:
        return 0
    if 256 * K + K >= 2 ** 31:
        return 0
    return int(rank_pad in RANK_PADS)


OK_TABLE = list(itertools.product((0, 64, 511, 512, 513, 32760, 2 ** 30), (0, 8, 12, 520, 5120), (0, 64, 128, 192, 640, 13824, 2 ** 23),
                                  (0, 16, 32, 48, 64, 96, 128, 256)))


def _gen(*key):
    seed = 28
    for v in key:
        seed = (seed * 1000003 + int(v)) % (2 ** 31)
    return torch.Generator().manual_seed(seed)


def integer_inputs(M, N, K, rp, r, scale, seed=0):
    """CPU operands of the exact class: a8 / w8 as e4m3 tensors of small integers, everything else bf16 integers (t / up zero past r)."""
    g = _gen(M, N, K, rp, r, seed)

    def ints(shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=g).float()
    a, w = ints((M, K), -4, 4), ints((N, K), -4, 4)
    d = dict(a8=a.to(G.E4M3), w8=w.to(G.E4M3), row_scale=2.0 ** ints((M,), -3, 1), bias=ints((N,), -8, 8).to(BF),
             t=torch.zeros(M, rp, dtype=BF), up=torch.zeros(N, rp, dtype=BF), resid=ints((M, N), -4, 4).to(BF),
             gate=ints((N,), -4, 4).to(BF), scale=scale, acc=(a.double() @ w.double().t()))
    d["t"][:, :r] = ints((M, r), -3, 3).to(BF)
    d["up"][:, :r] = ints((N, r), -3, 3).to(BF)
    return d


def _band(shape, g, lo=-3, hi=1):
    """bf16 values with random 8-bit significands and exponents in [lo, hi], random signs."""
    sig = 1.0 + torch.randint(0, 128, shape, generator=g).double() / 128.0
    return (sig * 2.0 ** torch.randint(lo, hi + 1, shape, generator=g).double() * (1 - 2 * torch.randint(0, 2, shape, generator=g))).to(BF)


def selector_inputs(M, N, K, rp, r, scale, seed=0):
    """The selector class: every row of a8 has ONE non-zero, a signed power of two, at a column of its own choice, and so has every row
    of t (inside the true rank) — acc[m, n] is one scaled element of w8 and d[m, n] one scaled element of up, whatever the order of the
    sums, while w8 (random e4m3 codes), up, bias, resid and gate carry full random significands.  Every fp32 operation of the kernel
    then has an exactly known result, which the chain rounds as the kernel does (fp64 exact -> fp32 -> bf16)."""
    g = _gen(M, N, K, rp, r, seed, 1)
    a = torch.zeros(M, K)
    a[torch.arange(M), torch.randint(0, K, (M,), generator=g)] = (2.0 ** torch.randint(-2, 3, (M,), generator=g).float()) * (1 - 2 * torch.randint(0, 2, (M,), generator=g)).float()
    w8 = _band((N, K), g, -3, 1).to(G.E4M3)
    t = torch.zeros(M, rp, dtype=BF)
    t[torch.arange(M), torch.randint(0, r, (M,), generator=g)] = ((2.0 ** torch.randint(-2, 3, (M,), generator=g).float()) * (1 - 2 * torch.randint(0, 2, (M,), generator=g)).float()).to(BF)
    up = torch.zeros(N, rp, dtype=BF)
    up[:, :r] = _band((N, r), g)
    return dict(a8=a.to(G.E4M3), w8=w8, row_scale=2.0 ** torch.randint(-3, 2, (M,), generator=g).float(), bias=_band((N,), g), t=t, up=up,
                resid=_band((M, N), g), gate=_band((N,), g), scale=scale, acc=a.double() @ w8.float().double().t())


EXACT = dict(integers=integer_inputs, selector=selector_inputs)


def chain(d, epi):
    """The fp64 chain of the header's formula on an input dict -> the bf16 result as fp64.  y0 is rounded as the kernel rounds it: the
    exact acc * row_scale + bias (one fma) to fp32, then to bf16."""
    y0 = LR.rb32(d["acc"] * d["row_scale"].double()[:, None] + d["bias"].double())
    ref, _ = LR.chain(y0, d["t"], d["up"], d["scale"], epi, d["resid"] if epi in LR.HAS_R else None,
                      d["gate"] if epi == G.EPI_GATE_RESID else None)
    return ref.out


def restate_f32(d, epi, fault=None):
    """The formula in fp32 torch operations, with the stated faults of the kernel's own steps (the CPU test shows each one leaves the
    exact class's equality): `scale_on_y0` — scale applied to y0 as well; `up_before_row_scale` — the up term added before the row
    scale; `neighbour_row` — row m reads t[m - 1]; `no_update` — the adapter's term missing."""
    a = torch.tensor(d["scale"], dtype=torch.float32)
    acc = d["acc"].float()
    t = d["t"].float()
    if fault == "neighbour_row":
        t = t.roll(1, 0)
    dd = (t @ d["up"].float().t()).to(BF).float()
    s = (a * dd).to(BF).float()
    rs = d["row_scale"].float()[:, None]
    if fault == "up_before_row_scale":
        y = (((acc + s) * rs + d["bias"].float()).to(BF)).float()
    else:
        y0 = (acc * rs + d["bias"].float()).to(BF).float()
        if fault == "scale_on_y0":
            y0 = (a * y0).to(BF).float()
        y = y0 if fault == "no_update" else (y0 + s).to(BF).float()
    if epi == G.EPI_GATE_RESID:
        return (d["resid"].float() + (d["gate"].float() * y).to(BF).float()).to(BF).double()
    if epi == G.EPI_RESID:
        return (d["resid"].float() + y).to(BF).double()
    if epi == G.EPI_MUL:
        return (y * d["resid"].float()).to(BF).double()
    assert epi == G.EPI_BIAS
    return y.double()


FAULTS = ("scale_on_y0", "up_before_row_scale", "neighbour_row", "no_update")


# ---------------------------------------------------------------------------------------------------------------------
# the tape: trainable adapters beside a FROZEN fp8 block (training.DiTBlockFn under lora.set_beside_fp8 + training.set_fp8_frozen)
# * fp64: the oracle's block with every Linear y = SteLinear(x, W, b) + s (x A^T) B^T — fp8_train_refs' straight-through fp8 layer
#   on W-hat plus peft's unmerged term on the UNQUANTISED x — differentiated by autograd: dx, dA, dB; the base weights get none.
# * fp32 restatement: lora_train_refs' adapted stages inside fp8_train_refs' fp8 layers (the adapters' GEMMs stay bf16: their
#   operands are not among the fp8 weights), orders 0 and 1.
# * the row statistic and its groups are lora_train_refs' (dx behind adapters: "dx_lora"); TAPE_ROW_WORST is the order-1 restatement's
#   worst ratio over tape_cases(), measured by tests/test_fp8_lora_cpu.py::test_tape_row_worst_reproduces; the device's bar is 1.25 x it.
import contextlib  # noqa: E402

TAPE_FAULTS = ("adapter_reads_dequantised_x", "no_adapter_in_dx", "dA_from_quantised_x", "dx_from_master")


def tape_cases():
    """lora_train_refs' block cases (64 / 65 / 130 / 72 tokens: every adapted layer by two launches) and one of 520 tokens, grid
    (1, 20, 26), rank 33: the token count from which the forward and the tape's recompute run gf_gemm_fp8_lora."""
    import lora_train_refs as LT
    return LT.block_cases() + [dict(name="tiny-520-7-r33", cfg="TINY", grid=(1, 20, 26), ctx_len=7, prescale=True, seed=106, rank=33, scaling=0.7,
                                    init="gauss")]


def adapted_fp8_grads_ref(cfg, sd, adapters, x, ctx, t_mod, dout, grid):
    """(dx, {"<layer>.lora_A.<i>" / "lora_B.<i>": gradient}, out) in fp64."""
    import fp8_train_refs as FT
    from oracle import wan_oracle as wo
    plain = wo._lin
    with torch.enable_grad():
        lo = {}
        for layer, ads in adapters.items():
            for i, (down, up, s) in enumerate(ads):
                lo[f"{layer}.lora_A.{i}"], lo[f"{layer}.lora_B.{i}"] = down.double().requires_grad_(True), up.double().requires_grad_(True)

        def lin(xx, sd_, name):
            y = FT.SteLinear.apply(xx, sd_[name + ".weight"], sd_.get(name + ".bias"))
            for i, (_, _, s) in enumerate(adapters.get(name, ())):
                y = y + LR.f32(s) * ((xx @ lo[f"{name}.lora_A.{i}"].t()) @ lo[f"{name}.lora_B.{i}"].t())
            return y
        wo._lin = lin
        try:
            xd = x.double()[None].requires_grad_(True)
            fr = wo.rope_freqs_3d(cfg["dim"] // cfg["num_heads"], *grid)
            y = wo.dit_block(xd, ctx.double()[None], t_mod.double(), fr, {k: v.double() for k, v in sd.items()}, "", cfg["num_heads"], cfg["eps"])
            y.backward(dout.double()[None])
        finally:
            wo._lin = plain
    return xd.grad[0], {k: v.grad for k, v in lo.items()}, y.detach()[0]


def adapted_fp8_chain(cfg, sd, adapters, x, ctx, t_mod, dout, grid, order=0, prescale=True, fault=None):
    """(dx bf16, {adapter gradient name: bf16}, out bf16) of the tape, restated in fp32; `fault`: one of TAPE_FAULTS' wrong lines.
    tape_refs' stages are module-level names looked up at call time, so the forward and the backward may run under different stages:
    `no_adapter_in_dx` runs block_fwd with the adapters' stages and block_bwd with the base tape alone (no adapter gradients result)."""
    import fp8_train_refs as FT
    import lora_train_refs as LT
    import tape_refs as TP
    assert fault is None or fault in TAPE_FAULTS, fault
    lo = {}
    with _mfma_model_up_to(TAPE_MFMA_MODEL_MAX), FT.fp8_layers(FT.linear_weights(sd), "dx_from_master" if fault == "dx_from_master" else None):
        with LT._adapted_stages(sd, adapters, lo), _dequantised_reads(adapters, fault):
            s = TP.block_fwd(cfg, sd, x, ctx, t_mod, grid, order, prescale)
            if fault != "no_adapter_in_dx":
                dx, _ = TP.block_bwd(s, dout)
        if fault == "no_adapter_in_dx":
            dx, _ = TP.block_bwd(s, dout)
    return dx, dict(lo), s.out


# Order 0 states the fp8 MFMA's own accumulator (gemm_refs.mfma_fp8) wherever that is affordable on the host; fp8_train_refs draws the line
# at M N K = 2^26, which every GEMM of its own cases is under.  The 520-token case's FFN GEMMs are 520 x 512 x 256 = 1.02 x 2^26: left
# to exact fp32 sums they make order 0 a draw of ANOTHER arithmetic than the device's in two layers of ten, and every gradient behind
# them inherits the difference.  The tape's restatement therefore models up to 2^27 (about a second more on the host).
TAPE_MFMA_MODEL_MAX = 2 ** 27


@contextlib.contextmanager
def _mfma_model_up_to(limit):
    import fp8_train_refs as FT
    old, FT.MFMA_MODEL_MAX = FT.MFMA_MODEL_MAX, max(FT.MFMA_MODEL_MAX, limit)
    try:
        yield
    finally:
        FT.MFMA_MODEL_MAX = old


@contextlib.contextmanager
def _dequantised_reads(adapters, fault):
    """Entered INSIDE lora_train_refs._adapted_stages, whose stages it wraps and puts back.  `dA_from_quantised_x`: the adapters'
    gradient stage (linear_dw, which takes t for dB and x for dA from its input) is handed x-hat * scale, the dequantised fp8 input.
    `adapter_reads_dequantised_x`: that, and the forward's t = gemm(x-hat * scale, A) in every layer that goes through `_lin` (all but
    cross_attn.o, whose residual form goes through `_gemm`).  Any other fault: nothing."""
    import fp8_train_refs as FT
    import tape_refs as TP
    if fault not in ("adapter_reads_dequantised_x", "dA_from_quantised_x"):
        yield
        return
    lin0, gemm0, dw0 = TP._lin, TP._gemm, TP.linear_dw          # the adapted stages (over the fp8 layers)

    def deq(a):
        return FT.dequant(*FT.fwd_codes(a)).to(BF)

    def _lin(xin, sd_, pre, order):
        y = gemm0(xin, sd_[pre + ".weight"], sd_[pre + ".bias"], order)
        for down, up, s in adapters.get(pre, ()):
            y = LR.restate(y, gemm0(deq(xin), down, None, order), up, s)
        return y

    if fault == "adapter_reads_dequantised_x":
        TP._lin = _lin
    TP.linear_dw = lambda dy, xin, order=0, fault=None: dw0(dy, deq(xin), order, fault)
    try:
        yield
    finally:
        TP._lin, TP.linear_dw = lin0, dw0


# measured: 9.955 (lora_up) at tiny-130-7-r4 (a row of dB on cross_attn.k / v is one sum over seven context rows with four live
# columns); 8.035 (lora_down) and 1.475 (dx_lora) at tiny-520-7-r33
TAPE_ROW_WORST = {"lora_up": 9.96, "lora_down": 8.04, "dx_lora": 1.48}


def tape_bars():
    import lora_train_refs as LT
    return {**LT.lora_bars(), **{k: 1.25 * v for k, v in TAPE_ROW_WORST.items()}}
