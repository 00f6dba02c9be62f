"""Training through frozen fp8 blocks, the part that needs no GPU: the header's two declarations, the gradient quantiser's restatement
on the rows that sit on its contract's edges, the measured bars of tests/fp8_train_refs.py (the order-1 restatement against fp64 autograd
of the straight-through fp8 block), the stated faults outside those bars, and the refusal rules of dit.refuse_training and
scripts/train.py::check_args under both states of training.set_fp8_frozen.  `pytest -s` prints every measured ratio."""
import ctypes
import functools
import importlib.util
import math
import os
import re

import pytest
import torch

import fp8_train_refs as F
import tape_refs as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


@pytest.fixture(autouse=True)
def _switch_restored():
    from goal_force_amd import training
    old = training.set_fp8_frozen(False)
    yield
    training.set_fp8_frozen(old)


# ---------------------------------------------------------------------------------------------------------------------
# the header
def test_header_declares_the_two_entry_points_and_keeps_the_abi_revision():
    from goal_force_amd import _lib
    with open(os.path.join(ROOT, "include", "goalforce.h")) as f:
        text = f.read()
    decl = _lib.parse_header(text)
    p, i64, fp = ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p
    assert decl["gf_quant_fp8_grad"][0] is ctypes.c_int and decl["gf_cast_fp8_t"][0] is ctypes.c_int
    assert [ctypes.sizeof(t) for t in decl["gf_quant_fp8_grad"][1]] == [ctypes.sizeof(t) for t in (p, p, fp, i64, i64, i64, i64, p)]
    assert [ctypes.sizeof(t) for t in decl["gf_cast_fp8_t"][1]] == [ctypes.sizeof(t) for t in (p, i64, p, i64, i64, i64, p)]
    flat = " ".join(text.split())
    assert ("GF_API int gf_quant_fp8_grad(const void* x, void* out8, float* scale, int64_t rows, int64_t dim, int64_t x_stride, "
            "int64_t out_stride, void* stream);") in flat
    assert "GF_API int gf_cast_fp8_t(const void* w, int64_t ldw, void* out8, int64_t ldo, int64_t N, int64_t K, void* stream);" in flat
    assert re.search(r"#define GF_ABI_VERSION (\d+)", text).group(1) == "20"


# ---------------------------------------------------------------------------------------------------------------------
# the quantiser's restatement
@pytest.mark.parametrize("dim", [8, 136])
def test_quantiser_restatement_on_the_hand_made_rows(dim):
    x, notes = F.hand_rows(dim)
    codes, scale = F.quant_grad_ref(x)
    assert codes.dtype == torch.uint8 and codes.shape == x.shape and scale.dtype == torch.float32
    amax = x.double().abs().amax(1)
    for r, (what, e) in enumerate(notes):
        if e is None:
            assert math.isnan(float(scale[r])) and not bool(codes[r].any()), what
            continue
        assert float(scale[r]) == 2.0 ** e, (what, float(scale[r]), e)
        a = float(amax[r])
        if a == 0:
            continue
        # the contract's sentence, in exact arithmetic (a power of two times a double)
        assert a * 2.0 ** -e <= 448.0, what
        assert e == -126 or a * 2.0 ** -(e - 1) > 448.0, what
        # one rounding: the codes are e4m3 of the exact quotient, and never the NaN code
        exact = (x[r].double() * 2.0 ** -e).float()
        assert torch.equal(codes[r], exact.to(F.E4M3).view(torch.uint8)), what
        assert not bool(((codes[r] & 0x7F) == 0x7F).any()), what
    by = {what: r for r, (what, _) in enumerate(notes)}
    tie = F.dequant(codes, scale)[by["e4m3 ties"]][:6].tolist()
    assert tie == [256.0, 16.0, -20.0, 2 * 2.0 ** -9, 0.0, -2 * 2.0 ** -9], tie                   # to even, subnormals included
    z = codes[by["zero row"]]
    assert int(z[1]) == 0x80 and not bool(z[torch.arange(dim) != 1].any()), "the zero row keeps the cast's codes of +-0"
    sub = F.dequant(codes, scale)[by["bf16 subnormals: e clamps at -126"]][:4].double()
    want = (x[by["bf16 subnormals: e clamps at -126"]][:4].double() * 2.0 ** 126).float().to(F.E4M3).float().double() * 2.0 ** -126
    assert torch.equal(sub, want) and float(sub[0]) != 0.0, "bf16 subnormals are quantised in the window 2^-126 opens, not flushed"
    big = F.dequant(codes, scale)[by["amax near 3e38"]]
    assert math.isfinite(float(big[0])) and abs(float(big[0]) / float(x[by["amax near 3e38"]][0]) - 1) <= 2.0 ** -4


def test_quantiser_restatement_is_the_e4m3_rounding_of_the_gradient_in_a_shifted_window():
    """Scaling a row by a power of two scales its scale and leaves its codes; the forward quantiser's clamp loses the same row."""
    x = F.gauss_rows(8, 256, seed=3)
    codes, scale = F.quant_grad_ref(x)
    c2, s2 = F.quant_grad_ref((x.float() * 2.0 ** -20).to(BF))
    assert torch.equal(codes, c2) and torch.equal(scale * 2.0 ** -20, s2)
    small = x[0:1]                                                    # magnitude 2^-30
    assert not bool(F.fwd_codes(small)[0].view(F.E4M3).float().any()) and bool(codes[0].any())


# ---------------------------------------------------------------------------------------------------------------------
# the bars: measured on the order-1 restatement, asserted to reproduce
CASES = {c["name"]: c for c in T.cases()}


@functools.lru_cache(maxsize=None)
def _block(name):
    import gen_inputs as gi
    case = CASES[name]
    cfg, sd, x, ctx, t_mod, dout = T.case_inputs(case, gi)
    ref = F.block_grads_ref(cfg, sd, x, ctx, t_mod, dout, case["grid"])
    c0 = F.block_chain_fp8(cfg, sd, x, ctx, t_mod, dout, case["grid"], 0, case["prescale"])[1]
    return (cfg, sd, x, ctx, t_mod, dout), ref, c0


@functools.lru_cache(maxsize=None)
def _model(zero):
    import gen_inputs as gi
    cfg, inp = gi.TINY, gi.train_inputs()
    dit_sd, cn_sd = gi.dit_sd(cfg, seed=41), gi.controlnet_sd(cfg, 2, seed=42, zero_convs_zero=zero)
    args = (cfg, dit_sd, cn_sd, 2, inp, gi.TRAIN_TIMESTEP_ID)
    return args, F.model_grads_ref(*args), F.model_chain_fp8(*args, order=0)


def test_row_worst_fp8_reproduces():
    worst = {}
    for name, case in CASES.items():
        (cfg, sd, x, ctx, t_mod, dout), ref, c0 = _block(name)
        c1 = F.block_chain_fp8(cfg, sd, x, ctx, t_mod, dout, case["grid"], 1, case["prescale"])[1]
        st = T.row_stat("dx", c1, c0, ref)
        print(f"ROW restatement order 1, {name}: dx worst ratio {st['worst']:.4f} at {st['where']}")
        assert st["zero_bad"] == 0
        worst["dx"] = max(worst.get("dx", 0.0), st["worst"])
    for zero in T.MODEL_CASES:
        args, (loss_ref, g_ref, p_ref), (l0, c0, p0) = _model(zero)
        l1, c1, _ = F.model_chain_fp8(*args, order=1)
        by_group = T.worst_by_group(T.measure(c1, c0, g_ref, True), True)
        bar = F.loss_bar(loss_ref, p_ref, p0, args[4])
        print(f"ROW restatement order 1, whole tape zero_convs_zero={zero}: {by_group}; loss fp64 {loss_ref:.7f} orders {l0:.7f} {l1:.7f} bar +-{bar:.2e}")
        assert abs(l0 - loss_ref) <= bar and abs(l1 - loss_ref) <= bar and bar <= 0.1 * loss_ref
        for k, v in by_group.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("ROW_WORST_FP8 measured:", {k: round(v, 4) for k, v in worst.items()})
    assert set(worst) == set(F.ROW_WORST_FP8)
    for k, v in worst.items():
        assert abs(v - F.ROW_WORST_FP8[k]) <= 0.005 * F.ROW_WORST_FP8[k] + 0.005, f"{k}: measured {v:.4f}, the helper states {F.ROW_WORST_FP8[k]}"
    assert F.ROW_BAR_FP8 == {k: 1.25 * v for k, v in F.ROW_WORST_FP8.items()}


@pytest.mark.parametrize("fault", F.FAULTS)
def test_every_stated_fault_lands_outside_the_bar(fault):
    (cfg, sd, x, ctx, t_mod, dout), ref, c0 = _block(T.BASE_CASE)
    case = CASES[T.BASE_CASE]
    sc = F.FAULT_DOUT_SCALE if fault in ("dy_min1_clamp", "dy_twice") else 1.0
    d = (dout.float() * sc).to(BF)
    if sc != 1.0:       # the right chain at a power-of-two multiple of the upstream gradient is that multiple of itself, exactly
        assert torch.equal(F.block_chain_fp8(cfg, sd, x, ctx, t_mod, d, case["grid"], 0, case["prescale"])[1].float(), c0.float() * sc)
    got = F.block_chain_fp8(cfg, sd, x, ctx, t_mod, d, case["grid"], 0, case["prescale"], fault=fault)[1]
    st = T.row_stat("dx", got, (c0.float() * sc).to(BF), ref * sc)
    print(f"FAULT {fault}: worst ratio {st['worst']:.3f} at {st['where']} (bar {F.ROW_BAR_FP8['dx']:.3f})")
    assert st["worst"] > F.ROW_BAR_FP8["dx"], f"{fault} passes: {st}"


def test_the_fp64_reference_is_the_straight_through_fp8_block():
    """SteLinear: the oracle's fp8_linear as value; W8 (not the master, not the transposed one) as the weight of dX; no dW."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn((5, 256), generator=g).to(BF).double().requires_grad_(True)
    w = (torch.randn((128, 256), generator=g) / 16).to(BF).double().requires_grad_(True)
    b = torch.randn(128, generator=g).to(BF).double()
    dy = torch.randn((5, 128), generator=g).double()
    with torch.enable_grad():
        y = F.SteLinear.apply(x, w, b)
        y.backward(dy)
    from oracle import fp8_oracle as fo
    x8, s = fo.quantize_activation(x.detach())
    w8 = w.detach().to(F.E4M3).double()
    assert torch.equal(y.detach(), (x8.double() @ w8.t()) * s.double() + b)
    assert torch.equal(x.grad, dy @ w8) and w.grad is None
    assert not torch.equal(x.grad, dy @ w.detach())


# ---------------------------------------------------------------------------------------------------------------------
# device-free: the refusal rules and the script's arguments
def _cpu_block(fp8=True):
    from goal_force_amd.dit import DiTBlock
    blk = DiTBlock(False, 256, 2, 512, 1e-6).to(BF)
    for p in blk.parameters():
        p.requires_grad_(False)
    if fp8:
        for m in blk.modules():
            if isinstance(m, torch.nn.Linear):
                m._gf_w8 = torch.zeros(1)                      # the copy enable_fp8 would hang there; refuse_training runs no kernel
    return blk


def test_refuse_training_under_both_switch_states():
    from goal_force_amd import dit, training
    from goal_force_amd._lib import GoalForceError
    old_message = "training through an enable_fp8 block is refused: call enable_fp8(module, False) first"
    blk = _cpu_block()
    assert training.FP8_FROZEN is False and training.set_fp8_frozen(False) is False
    with pytest.raises(GoalForceError) as e:                                  # off: word for word what it was
        dit.refuse_training(blk, training.FP8_FROZEN)
    assert str(e.value) == old_message
    with pytest.raises(GoalForceError) as e:
        dit.refuse_training(blk)
    assert str(e.value) == old_message
    assert training.set_fp8_frozen(True) is False and training.FP8_FROZEN is True
    dit.refuse_training(blk, training.FP8_FROZEN)                             # on: a frozen fp8 block is accepted
    dit.refuse_training(_cpu_block(fp8=False), training.FP8_FROZEN)           # and a bf16 block as ever
    blk.norm3.weight.requires_grad_(True)                                     # a trainable parameter: refused by its name
    with pytest.raises(GoalForceError, match=r"frozen blocks only.*the trainable parameter norm3\.weight"):
        dit.refuse_training(blk, training.FP8_FROZEN)
    blk.norm3.weight.requires_grad_(False)
    blk.self_attn.q.weight.requires_grad_(True)
    blk.ffn[2].bias.requires_grad_(True)
    with pytest.raises(GoalForceError, match=r"the trainable parameter self_attn\.q\.weight"):       # the first, in named_parameters' order
        dit.refuse_training(blk, training.FP8_FROZEN)
    # fp4, sage and sparse stay refused as today, switch on or off
    for on in (False, True):
        training.set_fp8_frozen(on)
        b4 = _cpu_block(fp8=on)                     # (off, a block carrying both kinds is refused as fp8 first, as it always was)
        b4.ffn[0]._gf_w4 = (torch.zeros(1), torch.zeros(1))
        with pytest.raises(GoalForceError, match=r"training through an enable_fp4 block is refused: call enable_fp4\(module, False\) first"):
            dit.refuse_training(b4, training.FP8_FROZEN)
        bs = _cpu_block(fp8=on)
        dit.enable_sage_attention(bs)
        with pytest.raises(GoalForceError, match="enable_sage_attention is refused"):
            dit.refuse_training(bs, training.FP8_FROZEN)
        bp = _cpu_block(fp8=on)
        dit.enable_sparse_attention(bp, lambda grid: None)
        with pytest.raises(GoalForceError, match="enable_sparse_attention is refused"):
            dit.refuse_training(bp, training.FP8_FROZEN)
    assert training.set_fp8_frozen(False) is True


def test_a_live_adapter_in_an_fp8_block_is_refused_with_the_switch_on():
    from goal_force_amd import dit, lora, training
    from goal_force_amd._lib import GoalForceError
    blk = _cpu_block(fp8=False)
    lora.add_trainable(blk, ["q"], 4)
    for m in blk.modules():
        if isinstance(m, torch.nn.Linear):
            m._gf_w8 = torch.zeros(1)
    training.set_fp8_frozen(True)
    with pytest.raises(GoalForceError, match="frozen blocks only"):
        dit.refuse_training(blk, training.FP8_FROZEN)


def test_fp8_weight_t_needs_an_fp8_layer_and_enable_fp8_false_drops_it():
    from goal_force_amd import dit
    from goal_force_amd._lib import GoalForceError
    blk = _cpu_block(fp8=False)
    with pytest.raises(GoalForceError, match="fp8_weight_t: the layer carries no fp8 copy"):
        dit.fp8_weight_t(blk.self_attn.q)
    lin = blk.self_attn.q
    lin._gf_w8, lin._gf_w8_key = torch.zeros(1), None
    lin._gf_w8t, lin._gf_w8t_key = torch.zeros(1), None
    dit.enable_fp8(blk, False)
    assert lin._gf_w8 is None and lin._gf_w8t is None


def _train_script():
    spec = importlib.util.spec_from_file_location("gf_train_script_fp8", os.path.join(ROOT, "scripts", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_check_args_with_and_without_lora_base_model():
    from goal_force_amd import training
    script = _train_script()
    base = ["--dataset_base_path", "x", "--control_signal_type", "canny_edge"]
    args = script.parser().parse_args(base + ["--trainable_models", "controlnet", "--enable_fp8_training"])
    assert args.enable_fp8_training is True
    script.check_args(args)                                                                    # accepted: frozen experts, a bf16 ControlNet
    assert script.parser().parse_args(base).enable_fp8_training is False
    assert not hasattr(training.wan_parser().parse_args(base), "enable_fp8_training")          # wan_parser is the reference's, untouched
    for more, msg in [(("--lora_base_model", "dit"), "--enable_fp8_training"),
                      (("--lora_base_model", "controlnet", "--trainable_models", "controlnet"), "--enable_fp8_training"),
                      (("--trainable_models", "controlnet,dit"), "--enable_fp8_training: the experts run fp8 and frozen"),
                      (("--trainable_models", "dit2"), "--enable_fp8_training: the experts run fp8 and frozen"),
                      ((), "--trainable_models controlnet is what the HIP training step differentiates")]:
        with pytest.raises(NotImplementedError, match=msg):
            script.check_args(script.parser().parse_args(base + ["--enable_fp8_training"] + list(more)))
    # the switch the flag throws: both experts enabled, the tape opened; without the flag nothing happens
    import types
    pipe = types.SimpleNamespace(dit=torch.nn.Identity(), dit2=torch.nn.Identity())
    assert script.enable_fp8_training(pipe, script.parser().parse_args(base)) == 0 and training.FP8_FROZEN is False
    assert script.enable_fp8_training(pipe, args) == 2 and training.FP8_FROZEN is True
