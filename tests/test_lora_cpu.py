"""LoRA adapters without a GPU: the rule for names against the reference's dictionaries (g21), the fp64 chain against the reference's
merged weights (g21), every device-free refusal, the two C declarations, the attach / detach / set_strength bookkeeping, and the
sensitivity of the two bars the GPU test holds the kernels to (tests/lora_refs.py; gemm_refs.judge): the fp32 restatement passes them
on every gauss input of tests/test_lora_gpu.py, each stated fault does not."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import gemm_refs as G
import lora_refs as LR
from forward_refs import bf16_steps, bits

BF = torch.bfloat16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_lora.npz")


@pytest.fixture(scope="module")
def g21():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def lora():
    from goal_force_amd import lora as _lora
    return _lora


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


# ---------------------------------------------------------------------------------------------------------------------
# names
def test_name_dict_is_the_references_on_the_golden_files(lora, g21):
    for load in range(len(LR.GOLDEN_LOADS)):
        keys = json.loads(str(g21[f"keys_{load}"]))
        want = {k: tuple(v) for k, v in json.loads(str(g21[f"name_dict_{load}"])).items()}
        got = lora.name_dict(dict.fromkeys(keys))
        assert got == want and list(got) == list(want), (load, got, want)
        assert set(LR.GOLDEN_TARGETS) <= set(got) and len(got) > len(LR.GOLDEN_TARGETS), "the files carry keys that match nothing"
        assert int(g21[f"updated_{load}"]) == len(LR.GOLDEN_TARGETS)
    # the files regenerate to the key lists the reference saw
    base = LR.golden_base_sd("gauss")
    for load in range(len(LR.GOLDEN_LOADS)):
        assert list(LR.golden_lora_sd(load, "gauss", base)) == json.loads(str(g21[f"keys_{load}"]))


def test_kohya_keys_match_nothing(lora):
    sd = {"lora_unet_blocks_0_self_attn_q.lora_up.weight": 0, "lora_unet_blocks_0_self_attn_q.lora_down.weight": 0,
          "lora_unet_blocks_0_self_attn_q.alpha": 0}
    assert lora.name_dict(sd) == {}


def test_plan_matches_the_models_linears_and_ignores_strays(lora, capsys):
    from goal_force_amd.dit import WanModel
    import gen_inputs as gi
    dit = WanModel(has_image_input=False, require_clip_embedding=False, **gi.TINY)
    base = LR.golden_base_sd("gauss")
    for load in range(len(LR.GOLDEN_LOADS)):
        todo = lora.plan(dit, LR.golden_lora_sd(load, "gauss", base))
        assert sorted(t[0] for t in todo) == sorted(LR.GOLDEN_TARGETS)
    # a lora_B key that matches no module is ignored whole, its missing partner included (the reference looks partners up for matched names only)
    stray = {**LR.golden_lora_sd(0, "gauss", base), "blocks.9.ffn.0.lora_B.weight": torch.ones(2, 2), "nowhere.lora_B.default.weight": torch.ones(2, 2)}
    assert sorted(t[0] for t in lora.plan(dit, stray)) == sorted(LR.GOLDEN_TARGETS)
    assert lora.load(dit, {"lora_unet_x.lora_up.weight": torch.zeros(2, 2), "nowhere.lora_B.weight": torch.ones(2, 2)}) == 0   # nothing matches: no device is needed
    assert capsys.readouterr().out.strip() == "0 tensors are updated by LoRA."


# ---------------------------------------------------------------------------------------------------------------------
# the chain against the reference's result
@pytest.mark.parametrize("cls", LR.GOLDEN_CLASSES)
def test_chain_against_the_references_merged_weights(g21, cls):
    refs, chains, _ = LR.golden_reference_weights(g21, cls)
    cap = float(g21["share_cap"])
    assert cap == 2.0 ** -12 and float(g21["cpu_share"]) <= cap
    worst = 0.0
    for load, (ref, ch) in enumerate(zip(refs, chains)):
        for n in LR.GOLDEN_TARGETS:
            if cls == "integers":
                assert torch.equal(bits(ref[n]), bits(ch[n])), f"integers load {load} {n}: the chain is not the reference's result"
            else:
                diff = bits(ref[n]) != bits(ch[n])
                worst = max(worst, float(diff.double().mean()))
                assert float(diff.double().mean()) <= cap and int(bf16_steps(ref[n], ch[n]).max()) <= 1, (load, n)
    print(f"g21 {cls}: worst share of elements where the reference differs from the chain {worst:.2e} (stored {float(g21['cpu_share']):.2e})")
    base = LR.golden_base_sd(cls)
    assert any(not torch.equal(refs[0][n], base[n + ".weight"]) for n in LR.GOLDEN_TARGETS)
    assert all(not torch.equal(refs[1][n], refs[0][n]) for n in LR.GOLDEN_TARGETS), "the second load stacks on the first"


# ---------------------------------------------------------------------------------------------------------------------
# refusals that need no device
class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.q = nn.Linear(16, 24)
        self.norm = nn.LayerNorm(16)
        self.sub = nn.Sequential(nn.Linear(16, 8), nn.GELU(), nn.Linear(8, 16))


def _pair(name, n, k, r, spelling="lora_B.weight"):
    return {f"{name}.{spelling}": torch.ones(n, r), f"{name}.{spelling}".replace("lora_B", "lora_A"): torch.ones(r, k)}


@pytest.mark.parametrize("entry", ["load", "attach"])
def test_refusals_by_name_before_any_weight_is_touched(lora, entry):
    from goal_force_amd._lib import GoalForceError
    net = _Net()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    call = (lambda sd, alpha=1.0: lora.load(net, sd, alpha)) if entry == "load" else (lambda sd, alpha=1.0: lora.attach(net, sd, alpha))
    good = _pair("sub.0", 8, 16, 4)
    cases = [
        ({"q.lora_B.weight": torch.ones(24, 4)}, r"'q\.lora_B\.weight' has no partner 'q\.lora_A\.weight'"),
        (_pair("norm", 16, 16, 4), r"addresses 'norm', a LayerNorm: only nn\.Linear"),
        ({"q.lora_B.weight": torch.ones(24, 4, 1, 1), "q.lora_A.weight": torch.ones(4, 16, 1, 1)}, r"must be 2-D"),
        (_pair("q", 23, 16, 4), r"'q' is \[24, 16\]: expected 'q\.lora_B\.weight' \[24, r\]"),
        (_pair("q", 24, 15, 4), r"expected 'q\.lora_B\.weight' \[24, r\] and 'q\.lora_A\.weight' \[r, 16\]"),
        ({"q.lora_B.weight": torch.ones(24, 4), "q.lora_A.weight": torch.ones(5, 16)}, r"\[r, 16\], got \(24, 4\) and \(5, 16\)"),
        (_pair("q", 24, 16, 257), r"rank 257: expected 1 <= r <= 256"),
        ({"q.lora_B.weight": torch.ones(24, 0), "q.lora_A.weight": torch.ones(0, 16)}, r"rank 0: expected 1 <= r <= 256"),
    ]
    for sd, msg in cases:
        with pytest.raises(GoalForceError, match=msg):
            call({**good, **sd})                       # (a good pair ahead of the bad one: it must not have been applied)
    for alpha in (math.inf, -math.inf, math.nan):
        with pytest.raises(GoalForceError, match="alpha must be finite"):
            call(good, alpha)
    with pytest.raises(GoalForceError, match="alpha must be a number"):
        call(good, "strong")
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    assert not any(lora.adapters(m) for m in net.modules())
    if entry == "load":                                # a good file on a CPU module: the merge has no CPU path, and says so
        with pytest.raises(GoalForceError, match=r"load_lora: 'sub\.0': the weight must be bf16 on the GPU"):
            call(good)
        assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_the_two_declarations_and_the_revision():
    import ctypes
    from goal_force_amd import _lib
    v, i64, f, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int
    assert _lib.ABI_VERSION == 20
    assert _lib.BINDINGS["gf_lora_merge"] == (i, [v, i64, v, i64, v, i64, i64, i64, i64, f, v])
    assert _lib.BINDINGS["gf_lora_up"] == (i, [v, i64, v, i64, v, i64, v, i64, i64, i64, i64, f, i, v, i64, v, v])


# ---------------------------------------------------------------------------------------------------------------------
# bookkeeping of the attached form
def test_attach_detach_set_strength_bookkeeping(lora):
    from goal_force_amd import dit
    from goal_force_amd._lib import GoalForceError
    net = dit.DiTBlock(False, 256, 2, 512).to(BF)
    q, f2 = net.self_attn.q, net.ffn[2]
    before = {k: v.clone() for k, v in net.state_dict().items()}
    epoch = dit._CACHE_EPOCH[0]
    g = torch.Generator().manual_seed(5)
    kb, ka = "diffusion_model.self_attn.q.lora_B.default.weight", "diffusion_model.self_attn.q.lora_A.default.weight"
    sd = {kb: torch.randn(256, 5, generator=g), ka: torch.randn(5, 256, generator=g),
          **{k: torch.randn(v.shape, generator=g) for k, v in _pair("ffn.2", 256, 512, 33).items()}, "nothing.lora_B.weight": torch.ones(2, 2),
          "nothing.lora_A.weight": torch.ones(2, 2)}
    assert lora.attach(net, sd, alpha=0.7) == 2 and dit._CACHE_EPOCH[0] == epoch + 1
    (ad,) = lora.adapters(q)
    assert (ad.name, ad.alpha, ad.rank) == ("default", 0.7, 5) and ad.down.shape == (32, 256) and ad.up.shape == (256, 32)
    assert ad.down.dtype == ad.up.dtype == BF
    assert torch.equal(ad.down[:5], sd[ka].to(BF)) and not bool(ad.down[5:].any())
    assert torch.equal(ad.up[:, :5], sd[kb].to(BF)) and not bool(ad.up[:, 5:].any())
    (ad2,) = lora.adapters(f2)
    assert ad2.rank == 33 and ad2.down.shape == (64, 512) and ad2.up.shape == (256, 64)
    assert not lora.adapters(net.ffn[0]) and lora.live(q) == [ad]
    with pytest.raises(GoalForceError, match="already carries an adapter named 'default'"):
        lora.attach(net, sd)
    assert lora.attach(net, sd, alpha=-1.0, name="style") == 2
    assert [a.name for a in lora.adapters(q)] == ["default", "style"] == [a.name for a in lora.live(q)]
    assert lora.set_strength(net, 0.0, "default") == 2 and [a.name for a in lora.live(q)] == ["style"]
    assert lora.set_strength(net, 2.5) == 4 and [a.alpha for a in lora.adapters(q)] == [2.5, 2.5]
    with pytest.raises(GoalForceError, match="alpha must be finite"):
        lora.set_strength(net, math.nan)
    assert lora.set_strength(net, 1.0, "nobody") == 0
    epoch = dit._CACHE_EPOCH[0]
    assert lora.detach(net, "default") == 2 and [a.name for a in lora.adapters(q)] == ["style"] and dit._CACHE_EPOCH[0] == epoch + 1
    assert lora.detach(net, "default") == 0 and dit._CACHE_EPOCH[0] == epoch + 1
    assert lora.detach(net) == 2 and not any(lora.adapters(m) for m in net.modules()) and not hasattr(q, "_gf_lora")
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items()) and list(net.state_dict()) == list(before)
    # a layer that carries a quantised copy takes no attached adapter
    q._gf_w8 = object()
    with pytest.raises(GoalForceError, match=r"lora\.attach: 'self_attn\.q' carries an enable_fp8 weight copy"):
        lora.attach(net, sd)
    assert not any(lora.adapters(m) for m in net.modules())
    # nor does a Linear outside the blocks, which launches its GEMM itself: the merged form is for those
    import gen_inputs as gi
    model = dit.WanModel(has_image_input=False, require_clip_embedding=False, **gi.TINY)
    for name, (n, k) in (("head.head", (64, 256)), ("text_embedding.0", (256, 64))):
        with pytest.raises(GoalForceError, match=rf"lora\.attach: '{name}' is not a Linear of a DiT block"):
            lora.attach(model, {**_pair("blocks.0.ffn.0", 512, 256, 4), **_pair(name, n, k, 4)})
    assert not any(lora.adapters(m) for m in model.modules())


def test_a_live_adapter_refuses_training(lora):
    from goal_force_amd import dit
    from goal_force_amd._lib import GoalForceError
    blk = dit.DiTBlock(False, 256, 2, 512).to(BF)
    sd = _pair("ffn.0", 512, 256, 4)
    lora.attach(blk, sd)
    with pytest.raises(GoalForceError, match=r"training through a block with a live LoRA adapter \(ffn\.0: 'default'\) is refused"):
        dit.refuse_training(blk)
    lora.set_strength(blk, 0)
    dit.refuse_training(blk)
    lora.set_strength(blk, 1)
    lora.detach(blk)
    dit.refuse_training(blk)


# ---------------------------------------------------------------------------------------------------------------------
# the bars: the restatement passes, the faults do not
def _merge_case(n, k, r, alpha):
    d = LR.merge_inputs("gauss", n, k, r, alpha)
    return d, LR.merge_chain(d)


def _fails(got, ref, K):
    a, b = G.passes(G.judge(got, ref, K))
    return not (a and b)


def test_restatement_passes_both_bars_on_every_gauss_merge_input():
    worst = (0.0, 0.0)
    for n, k, r, alpha in LR.MERGE_CASES:
        d, ref = _merge_case(n, k, r, alpha)
        for rev in (False, True):
            j = G.judge(LR.merge_restate(d, reverse=rev), ref, r)
            assert G.passes(j) == (True, True), ((n, k, r, alpha), G.describe(j))
            worst = (max(worst[0], j["share"]), max(worst[1], j["worst"]))
    print(f"merge restatement: worst differing share {worst[0]:.2e}, worst ratio of (b) {worst[1]:.2f}")


@pytest.mark.parametrize("fault", LR.FAULTS)
def test_each_merge_fault_is_outside_a_bar(fault):
    seen = 0
    for n, k, r, alpha in LR.MERGE_CASES:
        if alpha == 0.0 or (alpha == 1.0 and fault in ("alpha_bf16", "alpha_first", "no_first_rounding", "add_before_scale")):
            continue            # (alpha 1: the scale is exact and these four compute the chain itself)
        if (fault == "neighbour_row" and n < 2) or (fault == "down_transposed" and (r < 2 or k < 2)):
            continue            # (the fault does not exist at this shape)
        d, ref = _merge_case(n, k, r, alpha)
        assert _fails(LR.merge_restate(d, fault=fault), ref, r), f"{fault} passes both bars at {(n, k, r, alpha)}"
        seen += 1
    assert seen >= 5


def _up_case(case):
    M, N, rp, r, scale = case
    return LR.up_inputs("gauss", M, N, rp, r, scale)


def test_restatement_passes_both_bars_on_every_gauss_up_input():
    worst = (0.0, 0.0)
    for case in LR.UP_CASES:
        d = _up_case(case)
        for epi in G.EPIS:
            j = G.judge(LR.up_restate(d, epi), LR.up_chain(d, epi)[0], case[2])
            assert G.passes(j) == (True, True), (case, G.EPI_NAMES[epi], G.describe(j))
            worst = (max(worst[0], j["share"]), max(worst[1], j["worst"]))
    print(f"up restatement: worst differing share {worst[0]:.2e}, worst ratio of (b) {worst[1]:.2f}")


@pytest.mark.parametrize("fault", LR.FAULTS + LR.UP_FAULTS)
def test_each_up_fault_is_outside_a_bar(fault):
    seen = 0
    for case in LR.UP_CASES:
        M, N, rp, r, scale = case
        if scale == 0.0 or (scale == 1.0 and fault in ("alpha_bf16", "alpha_first", "no_first_rounding", "add_before_scale")):
            continue
        if (fault == "neighbour_row" and M < 2) or (fault == "down_transposed" and N < 2):
            continue
        d = _up_case(case)
        epis = {"epi_on_y0": (1, 2, 3, 4, 5), "gate_after_resid": (G.EPI_GATE_RESID,)}.get(fault, G.EPIS)
        for epi in epis:
            assert _fails(LR.up_restate(d, epi, fault=fault), LR.up_chain(d, epi)[0], rp), f"{fault} passes both bars at {case} {G.EPI_NAMES[epi]}"
        seen += 1
    assert seen >= 3
