"""LoRA adapters beside fp8 Linears, what needs no device: the two declarations, the switch lora.set_beside_fp8 and the refusals it
keeps or lifts, the option, ops.gemm_fp8_lora's device-free refusals, gf_gemm_fp8_lora_ok against its restatement, and the exact
class of tests/fp8_lora_refs.py: the fp32 restatement equals the fp64 chain on every input of the GPU test, each stated fault does
not."""
import pytest
import torch

import fp8_lora_refs as FL
import gemm_refs as G

BF = torch.bfloat16


@pytest.fixture
def lora():
    from goal_force_amd import lora as _lora
    old = _lora.set_beside_fp8(False)
    yield _lora
    _lora.set_beside_fp8(old)


def _pair(name, n, k, r, seed=3):
    g = torch.Generator().manual_seed(seed)
    return {f"{name}.lora_B.weight": torch.randn(n, r, generator=g), f"{name}.lora_A.weight": torch.randn(r, k, generator=g)}


def test_the_two_declarations_and_the_revision():
    import ctypes
    from goal_force_amd import _lib
    v, i64, f, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int
    assert _lib.ABI_VERSION == 20
    assert _lib.BINDINGS["gf_gemm_fp8_lora_ok"] == (i, [i64, i64, i64, i64])
    assert _lib.BINDINGS["gf_gemm_fp8_lora"] == (i, [v, i64, v, i64, v, v, v, i64, v, i64, i64, f, v, i64, i64, i64, i64, i, v, i64, v, v])


def test_ok_equals_its_restatement_on_a_table():
    from goal_force_amd import _lib
    lib = _lib.load()
    assert lib.gf_set_option(b"prefer_8wave", 0) == 0
    try:
        for M, N, K, rp in FL.OK_TABLE:
            assert lib.gf_gemm_fp8_lora_ok(M, N, K, rp) == FL.ok_py(M, N, K, rp), (M, N, K, rp)
        assert lib.gf_set_option(b"prefer_8wave", 1) == 0
        assert not any(lib.gf_gemm_fp8_lora_ok(*c) for c in FL.OK_TABLE)
    finally:
        lib.gf_set_option(b"prefer_8wave", 0)
    assert FL.ok_py(512, 8, 128, 32) == 1 and FL.ok_py(511, 8, 128, 32) == 0 and FL.ok_py(512, 8, 192, 32) == 0
    assert [FL.ok_py(640, 256, 256, rp) for rp in (0, 32, 48, 64, 96, 128)] == [0, 1, 0, 1, 0, 0]


def test_the_switch_returns_its_previous_value(lora):
    assert lora.beside_fp8() is False
    assert lora.set_beside_fp8(True) is False and lora.beside_fp8() is True
    assert lora.set_beside_fp8(1) is True and lora.set_beside_fp8(False) is True and lora.beside_fp8() is False


def test_option_defaults_on_and_round_trips():
    from goal_force_amd import ops
    assert ops.option("fp8_lora_fused") is True
    with ops.options(fp8_lora_fused=False):
        assert ops.option("fp8_lora_fused") is False
    assert ops.option("fp8_lora_fused") is True


def test_refusals_stand_with_the_switch_off_and_go_for_fp8_with_it_on(lora):
    from goal_force_amd import dit
    from goal_force_amd._lib import GoalForceError
    blk = dit.DiTBlock(False, 256, 2, 512).to(BF)
    q, f0 = blk.self_attn.q, blk.ffn[0]
    sd = {**_pair("self_attn.q", 256, 256, 4), **_pair("ffn.0", 512, 256, 4)}
    x = torch.zeros(8, 256, dtype=BF)
    # off: word for word
    q._gf_w8 = object()
    with pytest.raises(GoalForceError, match=r"lora\.attach: 'self_attn\.q' carries an enable_fp8 weight copy: attached adapters run on "
                                             r"bf16 layers only \(use the merged form, pipe\.load_lora, with quantised layers\)"):
        lora.attach(blk, sd)
    with pytest.raises(GoalForceError, match=r"lora\.add_trainable: 'self_attn\.q' carries an enable_fp8 weight copy"):
        lora.add_trainable(blk, "q", 4)
    q._gf_w8 = None
    assert lora.attach(blk, sd) == 2
    q._gf_w8 = object()
    with pytest.raises(GoalForceError, match=r"linear: an attached LoRA adapter \('default'\) on an enable_fp8 layer is refused: use the "
                                             r"merged form \(pipe\.load_lora\) with quantised layers, or lora\.detach first"):
        dit.linear(x, q)
    for m in blk.modules():
        if isinstance(m, torch.nn.Linear):
            m.weight.requires_grad_(False), m.bias.requires_grad_(False)
    for p in blk.parameters():
        p.requires_grad_(False)
    with pytest.raises(GoalForceError, match=r"open to frozen blocks only \(no weight gradient exists on the fp8 kernels\): this block has a "
                                             r"live LoRA adapter \(self_attn\.q: 'default'\)"):
        dit.refuse_training(blk, fp8_frozen=True)
    lora.detach(blk)
    # on: fp8 takes adapters, fp4 does not
    assert lora.set_beside_fp8(True) is False
    assert lora.attach(blk, sd) == 2 and [a.rank for a in lora.adapters(q)] == [4]
    with pytest.raises(GoalForceError, match="carries no bf16 source"):
        dit.linear(dit.QuantizedInput(None, data=torch.zeros(8, 256), scale=torch.ones(8)), q)
    with pytest.raises(GoalForceError, match="a QuantizedInput was handed to or asked of a layer with an attached LoRA adapter"):
        dit.linear(x, q, out=dit.QuantizedInput)
    lora.detach(blk)
    f0._gf_w4 = object()
    with pytest.raises(GoalForceError, match=r"lora\.attach: 'ffn\.0' carries an enable_fp4 weight copy"):
        lora.attach(blk, sd)
    f0._gf_w4 = None
    assert lora.attach(blk, sd) == 2
    f0._gf_w4 = object()
    with pytest.raises(GoalForceError, match=r"an attached LoRA adapter \('default'\) on an enable_fp4 layer is refused"):
        dit.linear(x, f0)


def test_a_quantized_input_keeps_its_bf16_source_only_when_built_from_one():
    from goal_force_amd import dit
    q = dit.QuantizedInput(None, data=torch.zeros(2, 8), scale=torch.ones(2))
    assert q.x2 is None and q.kind == "fp8"


def test_device_free_refusals_of_the_wrapper():
    from goal_force_amd import ops
    from goal_force_amd._lib import GoalForceError
    a8, w8 = torch.zeros(512, 128).to(G.E4M3), torch.zeros(8, 128).to(G.E4M3)
    t, up = torch.zeros(512, 32, dtype=BF), torch.zeros(8, 32, dtype=BF)
    with pytest.raises(GoalForceError, match=r"gemm_fp8_lora\.row_scale: required"):
        ops.gemm_fp8_lora(a8, None, w8, None, t, up, 1.0)
    with pytest.raises(GoalForceError, match="tensor must be on the GPU"):
        ops.gemm_fp8_lora(a8, torch.ones(512), w8, None, t, up, 1.0)


@pytest.fixture(scope="module")
def exact():
    out = []
    for make in FL.EXACT.values():
        for M, N, K, rp, r, scale in FL.CASES:
            d = make(M, N, K, rp, r, scale)
            out.append((d, {e: FL.chain(d, e) for e in FL.EXACT_EPIS}))
    return out


def test_restatement_equals_the_chain_on_every_exact_input(exact):
    for d, refs in exact:
        for e, ref in refs.items():
            assert torch.equal(FL.restate_f32(d, e), ref), (d["t"].shape, e)


@pytest.mark.parametrize("fault", FL.FAULTS)
def test_each_fault_leaves_the_equality(exact, fault):
    hit = 0
    for d, refs in exact:
        if d["scale"] == 0.0 or (fault == "scale_on_y0" and d["scale"] == 1.0):
            continue            # (a zero update hides the adapter's faults; scale 1 on y0 is the identity)
        hit += 1
        for e, ref in refs.items():
            assert not torch.equal(FL.restate_f32(d, e, fault), ref), (fault, d["t"].shape, e)
    assert hit >= 6


# ---------------------------------------------------------------------------------------------------------------------
# training adapters beside a frozen fp8 block
def test_refuse_training_takes_trainable_adapters_beside_fp8_only_under_both_switches(lora):
    from goal_force_amd import dit
    from goal_force_amd._lib import GoalForceError
    blk = dit.DiTBlock(False, 256, 2, 512).to(BF)
    for p in blk.parameters():
        p.requires_grad_(False)
    for m in blk.modules():
        if isinstance(m, torch.nn.Linear):
            m._gf_w8 = object()
    lora.set_beside_fp8(True)
    assert lora.add_trainable(blk, "q,ffn.0", 4) == 3
    dit.refuse_training(blk, fp8_frozen=True)                        # accepted: the adapters' parameters are the only trainable things
    with pytest.raises(GoalForceError, match="training through an enable_fp8 block is refused: call enable_fp8"):
        dit.refuse_training(blk)                                     # the tape's own switch is still needed
    blk.ffn[0].bias.requires_grad_(True)
    with pytest.raises(GoalForceError, match=r"open to frozen blocks only .*this block has the trainable parameter ffn\.0\.bias"):
        dit.refuse_training(blk, fp8_frozen=True)
    blk.ffn[0].bias.requires_grad_(False)
    lora.attach(blk, _pair("ffn.2", 256, 512, 4), name="frozen")
    with pytest.raises(GoalForceError, match=r"training through a block with a live LoRA adapter \(ffn\.2: 'frozen'\) is refused"):
        dit.refuse_training(blk, fp8_frozen=True)
    lora.detach(blk, "frozen")
    lora.set_beside_fp8(False)
    with pytest.raises(GoalForceError, match=r"open to frozen blocks only .*this block has the trainable parameter self_attn\.q\.lora_A"):
        dit.refuse_training(blk, fp8_frozen=True)                    # switch off: today's refusal (the adapter's own parameter is named)


def test_check_args_under_both_flag_states():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("gf_train_script", os.path.join(os.path.dirname(__file__), "..", "scripts", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    base = ["--dataset_base_path", "x", "--control_signal_type", "canny_edge", "--enable_fp8_training", "--lora_base_model"]
    for model in ("dit", "dit2", "controlnet"):
        with pytest.raises(NotImplementedError, match="--enable_fp8_training: trainable LoRA adapters run on bf16 layers only"):
            train.check_args(train.parser().parse_args(base + [model, "--trainable_models", ""]))
        args = train.parser().parse_args(base + [model, "--trainable_models", "", "--lora_beside_fp8"])
        assert args.lora_beside_fp8 is True
        train.check_args(args)
    with pytest.raises(NotImplementedError, match="may not name dit or dit2"):
        train.check_args(train.parser().parse_args(base + ["dit", "--trainable_models", "dit", "--lora_beside_fp8"]))
    assert train.parser().parse_args(base[:4]).lora_beside_fp8 is False


@pytest.fixture(scope="module")
def tape():
    import gen_inputs as gi
    import lora_train_refs as LT
    import tape_refs as TP
    out = {}
    for case in FL.tape_cases():
        cfg, sd, x, ctx, t_mod, dout = TP.case_inputs(case, gi)
        ads = LT.make_adapters(sd, case["rank"], case["scaling"], case["init"], seed=case["seed"])
        rdx, rg, _ = FL.adapted_fp8_grads_ref(cfg, sd, ads, x, ctx, t_mod, dout, case["grid"])
        c0 = FL.adapted_fp8_chain(cfg, sd, ads, x, ctx, t_mod, dout, case["grid"], 0, case["prescale"])
        out[case["name"]] = ((cfg, sd, ads, x, ctx, t_mod, dout, case), TP.with_dx(rdx, rg), TP.with_dx(c0[0], c0[1]))
    return out


def _chain(args, order=0, fault=None):
    import tape_refs as TP
    cfg, sd, ads, x, ctx, t_mod, dout, case = args
    c = FL.adapted_fp8_chain(cfg, sd, ads, x, ctx, t_mod, dout, case["grid"], order, case["prescale"], fault=fault)
    return TP.with_dx(c[0], c[1])


def test_tape_row_worst_reproduces(tape):
    """The order-1 restatement sits inside every bar on every input of the GPU test, and its worst ratios are the stored constants."""
    import lora_train_refs as LT
    import tape_refs as TP
    worst = {}
    for name, (args, ref, c0) in tape.items():
        stats = TP.measure(_chain(args, 1), c0, ref)
        assert not LT.lora_failures(stats, FL.tape_bars()), name
        for k, v in LT.lora_worst_by_group(stats).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("tape worst", worst)
    for k, v in FL.TAPE_ROW_WORST.items():
        assert worst[k] <= v <= 1.01 * worst[k] + 0.01, (k, worst[k], v)
    # peft's init: lora_B = 0 makes dA exactly zero, in the reference and in the restatement
    args, ref, c0 = tape["tiny-64-64-peft"]
    assert all(not bool(v.any()) for k, v in ref.items() if ".lora_A." in k) and all(not bool(v.any()) for k, v in c0.items() if ".lora_A." in k)


@pytest.mark.parametrize("fault", FL.TAPE_FAULTS)
def test_each_tape_fault_is_outside_a_bar(tape, fault):
    import lora_train_refs as LT
    import tape_refs as TP
    """Each stated fault leaves a bar on inputs of the GPU test (a bar is the worst over ALL cases, so a single case need not show every
    fault: the rank-4 cases with few rows per sum show the adapters' faults, the long-token cases the dx faults)."""
    caught = [name for name, (args, ref, c0) in tape.items() if not name.endswith("peft")
              and LT.lora_failures(TP.measure(_chain(args, 0, fault), c0, ref), FL.tape_bars())]
    print(f"tape fault {fault}: outside a bar on {caught}")
    assert len(caught) >= 2, (fault, caught)
