"""Trainable LoRA adapters on the device: lora.add_trainable, the adapters' part of training.DiTBlockFn, model_fn_train without a
ControlNet, launch_training_task's parameter list and checkpoints.  The references, the restatement and the bars are
tests/lora_train_refs.py's (tests/test_lora_train_cpu.py measures the bars on the CPU).

Every gradient — lora_A, lora_B of every adapter, the block's dx, and the 27 base gradients where the block trains them too — is held
per row and per column to the fp64 autograd of the block on W + s B A, at 1.25 x the restatement's own distance from it."""
import functools
import os

import pytest
import torch

import lora_refs as LR
import lora_train_refs as T
import tape_refs as TP

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CASES = {c["name"]: c for c in T.block_cases()}
TARGETS = "q,k,v,o,ffn.0,ffn.2"


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from goal_force_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _grad_enabled():
    with torch.enable_grad():
        yield


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------------
# the block fixture
@functools.lru_cache(maxsize=None)
def _case(name, second=False, base=False):
    """(inputs, adapters, fp64 reference, restatement of order 0) — computed once on the host and left unchanged."""
    import gen_inputs as gi
    case = CASES[name]
    cfg, sd, x, ctx, t_mod, dout = TP.case_inputs(case, gi)
    ads = T.make_adapters(sd, case["rank"], case["scaling"], case["init"], seed=case["seed"], second=(33, 0.7) if second else None)
    rdx, rg = T.adapted_grads_ref(cfg, sd, ads, x, ctx, t_mod, dout, case["grid"])
    c0 = T.adapted_block_chain(cfg, sd, ads, x, ctx, t_mod, dout, case["grid"], 0, case["prescale"])
    return (cfg, sd, x, ctx, t_mod, dout), ads, TP.with_dx(rdx, rg), TP.with_dx(c0[0], c0[1])


def _install(blk, ads, rank_of):
    """lora.add_trainable on every layer (a second adapter named "b" where the case has one), then the case's values written into the
    parameters' own storage."""
    from goal_force_amd import lora
    first = {layer: a[0] for layer, a in ads.items()}
    r0 = rank_of(first)
    assert lora.add_trainable(blk, TARGETS, r0, alpha=r0 * next(iter(first.values()))[2]) == 10
    two = [layer for layer, a in ads.items() if len(a) > 1]
    if two:
        s2 = ads[two[0]][1][2]
        assert lora.add_trainable(blk, [layer for layer in two], 33, alpha=33 * s2, name="b") == len(two)
    with torch.no_grad():
        for layer, lst in ads.items():
            have = lora.adapters(blk.get_submodule(layer))
            assert len(have) == len(lst) and all(ad.trainable for ad in have)
            for ad, (down, up, s) in zip(have, lst):
                assert ad.down.shape == down.shape and ad.up.shape == up.shape and abs(ad.alpha - s) < 1e-7, (layer, ad.alpha, s)
                ad.down.copy_(down.cuda())
                ad.up.copy_(up.cuda())
    return blk


def _block(cfg, sd):
    from goal_force_amd.dit import DiTBlock
    blk = DiTBlock(False, cfg["dim"], cfg["num_heads"], cfg["ffn_dim"], cfg["eps"])
    blk.load_state_dict(sd, strict=True)
    return blk.to(BF).cuda()


def _rope(cfg, grid):
    from goal_force_amd.dit import RopeTable, precompute_freqs_cis_3d
    return RopeTable.from_grid(precompute_freqs_cis_3d(cfg["dim"] // cfg["num_heads"]), *grid, "cuda")


def _run(ops, name, inputs, ads, train_base=False, level=None, monkeypatch=None):
    """One forward + backward of the adapted block -> ({gradient name: tensor on the CPU}, the forward's output, the block)."""
    from goal_force_amd import lora, training
    case = CASES[name]
    cfg, sd, x, ctx, t_mod, dout = inputs
    blk = _block(cfg, sd)
    for p_ in blk.parameters():
        p_.requires_grad_(train_base)
    _install(blk, ads, lambda first: case["rank"])
    if level is not None:
        monkeypatch.setattr(training, "KEEP_ATTENTION", True)
        monkeypatch.setattr(training, "KEEP_WIDE", False)
        monkeypatch.setattr(training, "KEEP_AUTO", True)
        training.set_keep_level(level)
    xc = x.cuda().requires_grad_(True)
    with ops.options(attn_q_prescale=case["prescale"]):
        y = training.block_forward(blk, xc, ctx.cuda(), t_mod.cuda(), _rope(cfg, case["grid"]))
        y.backward(dout.cuda())
    got = {"dx": xc.grad.cpu()}
    for layer, lst in ads.items():
        for i, ad in enumerate(lora.adapters(blk.get_submodule(layer))):
            assert ad.down.grad is not None and ad.up.grad is not None, f"{layer}: adapter {i} got no gradient"
            got[f"{layer}.lora_A.{i}"], got[f"{layer}.lora_B.{i}"] = ad.down.grad.cpu(), ad.up.grad.cpu()
    named = dict(blk.named_parameters())
    for n in TP.PARAM_NAMES:
        assert (named[n].grad is not None) == train_base, f"{n}: .grad {'missing' if train_base else 'set on a frozen weight'}"
        if train_base:
            got[n] = named[n].grad.cpu()
    return got, y.detach(), blk


def _assert_rows(got, c0, ref, what):
    stats = TP.measure(got, c0, ref)
    bars = T.lora_bars()
    for k, v in sorted(T.lora_worst_by_group(stats).items()):
        print(f"ROW {what} {k}: worst ratio {v:.3f} (bar {bars[k]:.3f})")
    fails = T.lora_failures(stats, bars)
    assert not fails, f"{what}: " + "; ".join(fails)


@pytest.mark.parametrize("name", [n for n in CASES if not n.endswith("peft")])
def test_adapter_gradients_and_dx_every_slice(ops, name):
    inputs, ads, ref, c0 = _case(name)
    got, _, _ = _run(ops, name, inputs, ads)
    assert set(got) == {"dx"} | {f"{layer}.lora_{ab}.0" for layer in T.LAYERS for ab in "AB"}
    _assert_rows(got, c0, ref, f"lora block {name}")


@pytest.mark.parametrize("level", ["none", "attn", "wide"])
def test_adapter_gradients_at_every_keep_level(ops, level, monkeypatch):
    name = "tiny-65-65-r33"
    inputs, ads, ref, c0 = _case(name)
    got, _, _ = _run(ops, name, inputs, ads, level=level, monkeypatch=monkeypatch)
    _assert_rows(got, c0, ref, f"lora block keep={level}")


def test_two_adapters_on_one_layer(ops):
    name = "tiny-65-65-r33"
    inputs, ads, ref, c0 = _case(name, second=True)
    assert len(ads["self_attn.q"]) == 2 and len(ads["ffn.2"]) == 2
    got, _, _ = _run(ops, name, inputs, ads)
    assert "self_attn.q.lora_A.1" in got and "ffn.2.lora_B.1" in got
    _assert_rows(got, c0, ref, "lora block, two adapters on self_attn.q and ffn.2")


def test_a_block_that_trains_its_own_weights_and_an_adapter(ops):
    """A ControlNet block: the 27 base gradients hold tape_refs' existing bars beside the adapters'."""
    name = "tiny-130-7-r4"
    inputs, ads, ref, c0 = _case(name)
    got, _, _ = _run(ops, name, inputs, ads, train_base=True)
    assert set(TP.PARAM_NAMES) <= set(got)
    _assert_rows(got, c0, ref, "lora block + its own 27 parameters")


def test_forward_is_the_attached_forward_and_peft_init_is_the_plain_block(ops):
    from goal_force_amd import lora, training
    name = "tiny-64-64-r4"
    inputs, ads, _, _ = _case(name)
    cfg, sd, x, ctx, t_mod, dout = inputs
    case = CASES[name]
    _, y_train, blk = _run(ops, name, inputs, ads)
    rope = _rope(cfg, case["grid"])
    args = (x.cuda(), ctx.cuda(), t_mod.cuda(), rope)
    with torch.no_grad():
        plain = _block(cfg, sd)
        y_plain = plain(*args).clone()
        att = _block(cfg, sd)
        lsd = {}
        for layer, [(down, up, s)] in ads.items():
            lsd[layer + ".lora_A.weight"], lsd[layer + ".lora_B.weight"] = down[:case["rank"]], up[:, :case["rank"]]
        assert lora.attach(att, lsd, alpha=case["scaling"]) == 10
        y_att = att(*args).clone()
        assert torch.equal(_bits(blk(*args)), _bits(y_att)), "a trainable adapter runs as an attached one of the same values"
        assert not torch.equal(y_att, y_plain)
        with ops.options(attn_q_prescale=case["prescale"]):
            y_plain_tape = training.block_forward(plain, *args[:3], rope).clone()
        assert not torch.equal(y_train, y_plain_tape)
    # peft's init: lora_B = 0 -> the plain block's bits, dA exactly 0, dB not
    pname = "tiny-64-64-peft"
    pin, pads, pref, pc0 = _case(pname)
    got, y0, _ = _run(ops, pname, pin, pads)
    assert torch.equal(_bits(y0), _bits(y_plain_tape)), "with lora_B = 0 the forward is the plain block's"
    for layer in T.LAYERS:
        assert not bool(got[f"{layer}.lora_A.0"].any()), f"{layer}: dA behind a zero lora_B is exactly zero"
        assert bool(got[f"{layer}.lora_B.0"][:, :CASES[pname]["rank"]].any()), f"{layer}: dB is zero"
    _assert_rows(got, pc0, pref, "lora block, peft init")


def test_refusals_by_message():
    from goal_force_amd import dit, lora, training
    from goal_force_amd._lib import GoalForceError
    import gen_inputs as gi
    cfg = gi.TINY
    model = dit.WanModel(has_image_input=False, require_clip_embedding=False, **cfg).to(BF).cuda()
    blk = model.blocks[0]
    with pytest.raises(GoalForceError, match=r"lora\.add_trainable: target 'nothing' matches no module"):
        lora.add_trainable(model, "q,nothing", 4)
    with pytest.raises(GoalForceError, match=r"lora\.add_trainable: 'head\.head' is not a Linear of a DiT block"):
        lora.add_trainable(model, ["q", "head.head"], 4)
    with pytest.raises(GoalForceError, match=r"lora\.add_trainable: rank 257: expected 1 <= r <= 256"):
        lora.add_trainable(model, "q", 257)
    for kind in ("fp8", "fp4"):
        getattr(dit, "enable_" + kind)(blk)
        with pytest.raises(GoalForceError, match=rf"lora\.add_trainable: 'blocks\.0\.\S+' carries an enable_{kind} weight copy"):
            lora.add_trainable(model, "o,ffn.0", 4)
        getattr(dit, "enable_" + kind)(blk, False)
    assert not lora.trainable(model) and not any(".lora_" in n for n, _ in model.named_parameters())
    # a frozen attached adapter stays refused in training; a trainable one beside it does not lift that
    sd = {"ffn.0.lora_B.weight": torch.ones(cfg["ffn_dim"], 4), "ffn.0.lora_A.weight": torch.ones(4, cfg["dim"])}
    lora.attach(blk, sd)
    lora.add_trainable(blk, "q", 4, name="t")
    with pytest.raises(GoalForceError, match=r"training through a block with a live LoRA adapter \(ffn\.0: 'default'\) is refused"):
        dit.refuse_training(blk)
    lora.detach(blk, "default")
    dit.refuse_training(blk)
    with pytest.raises(GoalForceError, match=r"already carries an adapter named 't'"):
        lora.add_trainable(blk, "q", 4, name="t")
    # an enable_fp8 block with a trainable adapter is refused by the tape
    dit.enable_fp8(blk)
    with pytest.raises(GoalForceError, match="training through an enable_fp8 block is refused"):
        dit.refuse_training(blk)
    dit.enable_fp8(blk, False)
    assert lora.detach(blk) == 2 and not any(".lora_" in n for n, _ in blk.named_parameters())
    with pytest.raises(GoalForceError, match="DiTBlockFn: 27 parameters for a block with 2 live trainable adapters"):
        lora.add_trainable(blk, "q", 4)
        x = torch.zeros((72, cfg["dim"]), dtype=BF, device="cuda")
        training.DiTBlockFn.apply(blk, None, x, x[:7], x[:6].view(1, 6, -1), *training._block_params(blk))


# ---------------------------------------------------------------------------------------------------------------------
# whole steps on the tiny models
def _tiny_pipe(n_cn, train_cn):
    import gen_inputs as gi
    from goal_force_amd.controlnet import ControlNet
    from goal_force_amd.dit import WanModel
    from goal_force_amd.pipeline import WanVideoPipeline
    cfg = gi.TINY
    dit_sd = gi.dit_sd(cfg, seed=41)
    dit = WanModel(has_image_input=False, require_clip_embedding=False, **cfg)
    dit.load_state_dict(dit_sd, strict=True)
    dit = dit.to(BF).cuda()
    cn = None
    if n_cn:
        cn = ControlNet(n_cn, dim=cfg["dim"], num_heads=cfg["num_heads"], ffn_dim=cfg["ffn_dim"])
        cn.load_state_dict(gi.controlnet_sd(cfg, n_cn, seed=42), strict=True)
        cn = cn.to(BF).cuda()
        for p_ in cn.parameters():
            p_.requires_grad_(train_cn)
    for p_ in dit.parameters():
        p_.requires_grad_(False)
    pipe = WanVideoPipeline.from_modules(dit, None, cn, None, device="cuda")
    pipe.scheduler.set_timesteps(1000, training=True)
    return pipe, dit_sd


def _loss(pipe, dev, tid):
    return pipe.training_loss(input_latents=dev["input_latents"], noise=dev["noise"], context=dev["context"], y=dev["y"],
                              control_signal_video_latents=dev["control"], timestep_id=tid)


def _predict(pipe, dev):
    from goal_force_amd.model_fn import model_fn_wan_video
    with torch.no_grad():
        ts = pipe.scheduler.timesteps[137:138].to(dtype=BF, device="cuda")
        return model_fn_wan_video(dit=pipe.dit, latents=dev["noise"], timestep=ts, context=dev["context"], y=dev["y"],
                                  controlnet=pipe.controlnet, control_signal_video_latents=dev["control"] if pipe.controlnet is not None else None).clone()


@pytest.mark.parametrize("n_cn", [0, 2])
def test_four_optimiser_steps_on_the_tiny_models(ops, n_cn, tmp_path):
    """model_fn_train(controlnet=None) and a step with a two-layer ControlNet: only adapter and ControlNet parameters carry gradients,
    the base weights are bit-identical after four steps, the loss moves, and the forward after the steps is that of a NEW model
    loaded with the updated values (no stale cache); the checkpoint holds peft's names at the true rank and loads into pipe.load_lora,
    lora.attach and --lora_checkpoint."""
    import gen_inputs as gi
    from goal_force_amd import lora, training
    from safetensors.torch import load_file
    torch.manual_seed(5)
    pipe, dit_sd = _tiny_pipe(n_cn, train_cn=True)
    dev = {k: v.cuda() for k, v in gi.train_inputs().items()}
    n = lora.add_trainable(pipe.dit, TARGETS, 4, alpha=4)
    assert n == 10 * gi.TINY["num_layers"]
    with torch.no_grad():            # lora_B away from zero, or the first steps would move nothing but lora_B
        for _, _, ad in lora.trainable(pipe.dit):
            ad.up[:, :ad.rank] = (0.05 * torch.randn((ad.up.shape[0], ad.rank))).to(BF).cuda()
    named = training.trainable_named_parameters(pipe, padded=True)
    assert sum(".lora_" in k for k in named) == 2 * n and all(k.startswith(("pipe.dit.blocks.", "pipe.controlnet.")) for k in named)
    assert (sum(k.startswith("pipe.controlnet.") for k in named) > 0) == bool(n_cn)
    base = {k: v.detach().clone() for k, v in pipe.dit.named_parameters() if ".lora_" not in k}
    before = _predict(pipe, dev)
    opt = training.AdamW(list(named.values()), lr=2e-3)
    losses = []
    for step in range(4):
        opt.zero_grad()
        loss = _loss(pipe, dev, gi.TRAIN_TIMESTEP_ID)
        loss.backward()
        if step == 0:
            ids = {id(p_) for p_ in named.values()}
            for model in (pipe.dit, pipe.controlnet):
                for k, p_ in (model.named_parameters() if model is not None else ()):
                    assert (p_.grad is not None) == (id(p_) in ids), f"{k}: gradient {'missing' if id(p_) in ids else 'on a frozen parameter'}"
        opt.step()
        losses.append(float(loss.detach()))
    print(f"PIN four LoRA steps (ControlNet layers {n_cn}): loss {losses}")
    assert all(torch.isfinite(torch.tensor(losses))) and min(losses[1:]) < losses[0]
    for k, v in pipe.dit.named_parameters():
        if ".lora_" not in k:
            assert torch.equal(_bits(v.detach()), _bits(base[k])), f"{k}: a frozen base weight moved"
    for _, _, ad in lora.trainable(pipe.dit):
        assert not bool(ad.down.detach()[ad.rank:].any()) and not bool(ad.up.detach()[:, ad.rank:].any()), "the rank's padding stayed zero"
    after = _predict(pipe, dev)
    assert not torch.equal(after, before)
    # a checkpoint through the logger: peft's names, the true rank
    args_prefix = "pipe.dit."
    logger = training.ModelLogger(str(tmp_path), remove_prefix_in_ckpt=args_prefix)
    path = logger.save_model(pipe, "step-4.safetensors")
    file_sd = load_file(path)
    lora_keys = [k for k in file_sd if ".lora_" in k]
    assert len(lora_keys) == 2 * n and all(k.startswith("blocks.") and k.endswith((".lora_A.default.weight", ".lora_B.default.weight")) for k in lora_keys)
    assert file_sd["blocks.0.self_attn.q.lora_A.default.weight"].shape == (4, gi.TINY["dim"])
    assert file_sd["blocks.0.ffn.0.lora_B.default.weight"].shape == (gi.TINY["ffn_dim"], 4)
    assert (len(file_sd) > len(lora_keys)) == bool(n_cn) and all(k.startswith("pipe.controlnet.") for k in file_sd if ".lora_" not in k)
    only_lora = {k: v for k, v in file_sd.items() if ".lora_" in k}
    # a NEW expert with the file attached (lora.attach) gives the trained forward bit for bit: no copy of the old values survived
    fresh, _ = _tiny_pipe(0, False)
    fresh.controlnet = pipe.controlnet
    assert lora.attach(fresh.dit, only_lora, alpha=1.0) == n
    assert torch.equal(_bits(_predict(fresh, dev)), _bits(after)), "the trained forward is not that of a new model with the updated values"
    # --lora_checkpoint: either key spelling restores the values bit for bit
    for spell in (lambda k: k, lambda k: k.replace(".default.weight", ".weight")):
        again, _ = _tiny_pipe(0, False)
        lora.add_trainable(again.dit, TARGETS, 4)
        got_n, unexpected = lora.load_trainable_state(again.dit, {spell(k): v for k, v in only_lora.items()} | {"blocks.9.ffn.0.lora_A.weight": torch.zeros(4, 8)})
        assert got_n == 2 * n and unexpected == ["blocks.9.ffn.0.lora_A.default.weight"]
        want = lora.trainable_state_dict(pipe.dit)
        have = lora.trainable_state_dict(again.dit)
        assert list(want) == list(have) and all(torch.equal(_bits(want[k]), _bits(have[k])) for k in want)
    # pipe.load_lora of the written file into a new expert: the merged forward, within test_lora_gpu's merged-vs-attached bar
    if n_cn == 0:
        from oracle import wan_oracle as wo
        merged, _ = _tiny_pipe(0, False)
        assert merged.load_lora(merged.dit, path, alpha=1.0) == n
        cpu = gi.train_inputs()
        ts = pipe.scheduler.timesteps[137:138].to(dtype=BF).double()
        names = sorted({k.split(".lora_")[0] for k in only_lora})
        sd_peft = {k: v.double() for k, v in dit_sd.items()}
        sd_mer = dict(sd_peft)
        for nm in names:
            up, down = only_lora[nm + ".lora_B.default.weight"], only_lora[nm + ".lora_A.default.weight"]
            sd_peft[nm + ".weight"] = sd_peft[nm + ".weight"] + up.double() @ down.double()
            sd_mer[nm + ".weight"] = LR.merged_weight(dit_sd[nm + ".weight"], up, down, 1.0).double()
        f64 = lambda sd: wo.model_fn(sd, dict(gi.TINY), cpu["noise"].double(), ts, cpu["context"].double(), cpu["y"].double())          # noqa: E731
        rel = lambda a, b: float((a.double().cpu() - b).norm() / b.norm())                                                          # noqa: E731
        e_att, e_mer = rel(after, f64(sd_peft)), rel(_predict(merged, dev), f64(sd_mer))
        print(f"PIN trained expert: attached forward rel-L2 from fp64 peft {e_att:.3e}; merged from the fp64 merged forward {e_mer:.3e}")
        assert e_att <= 1.25 * e_mer, (e_att, e_mer)


def test_launch_training_task_optimises_adapters_and_writes_pefts_keys(ops, tmp_path):
    """Four steps through the loop's forward= seam with fixed draws: the optimiser's list is the ControlNet's parameters and the
    adapters', the checkpoints carry both, and nothing to train is refused by name."""
    import types
    import gen_inputs as gi
    from goal_force_amd import lora, training
    from goal_force_amd._lib import GoalForceError
    from safetensors.torch import load_file
    pipe, _ = _tiny_pipe(0, False)
    dev = {k: v.cuda() for k, v in gi.train_inputs().items()}
    args = types.SimpleNamespace(learning_rate=1e-2, weight_decay=1e-2, dataset_num_workers=0, save_steps=2, num_epochs=1,
                                 gradient_accumulation_steps=1, output_path=str(tmp_path), remove_prefix_in_ckpt="pipe.dit.",
                                 control_signal_type="canny_edge", num_frames=5, max_grad_norm=1.0, controlnet_checkpoint=None)
    control = torch.zeros(5, 480, 832, 3, dtype=torch.uint8)
    items = [dict(video=[], control_video=control, file_id=str(i)) for i in range(4)]
    with pytest.raises(GoalForceError, match="launch_training_task: nothing to train"):
        training.launch_training_task(items, pipe, args=args, forward=lambda p_, d: None, shuffle=False)
    lora.add_trainable(pipe.dit, TARGETS, 4)
    seen = []

    def forward(p_, data):
        loss = _loss(p_, dev, gi.TRAIN_TIMESTEP_ID)
        seen.append(float(loss.detach()))
        return loss

    import datetime
    logger = training.launch_training_task(items, pipe, args=args, forward=forward, shuffle=False, now=datetime.datetime(2024, 1, 2, 3, 4, 5))
    assert logger.num_steps == 4 and len(seen) == 4 and seen[-1] != seen[0]
    files = sorted(os.listdir(logger.output_path))
    assert files == ["step-2.safetensors", "step-4.safetensors"]
    sd = load_file(os.path.join(logger.output_path, files[-1]))
    assert len(sd) == 20 * gi.TINY["num_layers"] and all(".lora_" in k and k.startswith("blocks.") for k in sd)
    assert bool(sd["blocks.0.self_attn.q.lora_B.default.weight"].any()), "lora_B left its zero initialisation"


def test_training_loop_vs_the_torch_restatement_of_peft_training(ops, tmp_path):
    """Four steps of launch_training_task through its forward= seam — fixed latents, noise and timesteps, no VAE — against g22
    (tests/golden/make_lora_train_golden.py): the oracle's model with peft's three-line forward, the reference's training_loss,
    torch.optim.AdamW, ConstantLR and clip_grad_norm_ on the CPU, in fp32 and in bf16.  Per-step loss and pre-clip gradient norm: no
    further from the fp32 run than its own bf16 run is, with the factor and floors of
    test_training_gpu.py::test_training_loop_vs_the_reference_launch_training_task (x 2; 2e-2 of the loss, 5e-2 of the norm)."""
    import datetime
    import types
    import numpy as np
    import gen_inputs as gi
    from conftest import GOLDEN
    from goal_force_amd import lora, training
    g = np.load(os.path.join(GOLDEN, "g22_lora_train.npz"))
    cfg = T.LOOP
    assert [int(v) for v in g["timestep_ids"]] == list(cfg["timestep_ids"])
    pipe, dit_sd = _tiny_pipe(0, False)
    assert lora.add_trainable(pipe.dit, cfg["targets"], cfg["rank"]) == 10 * gi.TINY["num_layers"]
    start = T.loop_adapters(gi.TINY, dit_sd)
    with torch.no_grad():
        for name, _, ad in lora.trainable(pipe.dit):
            a, b = start[name]
            ad.down[:ad.rank] = a.cuda()
            ad.up[:, :ad.rank] = b.cuda()
    dev = {k: v.cuda() for k, v in gi.train_inputs().items()}
    rec = {"loss": [], "lr": [], "norm": []}

    def forward(pipe_, data):
        loss = _loss(pipe_, dev, cfg["timestep_ids"][len(rec["loss"])])
        rec["loss"].append(float(loss.detach()))
        return loss

    real_end = training.ModelLogger.on_step_end

    def spy_end(self, pipe_, loss, learning_rate, grad_norm=None, save_steps=None):
        rec["lr"].append(learning_rate)
        rec["norm"].append(grad_norm)
        return real_end(self, pipe_, loss, learning_rate, grad_norm=grad_norm, save_steps=save_steps)

    args = types.SimpleNamespace(learning_rate=cfg["learning_rate"], weight_decay=cfg["weight_decay"], dataset_num_workers=0, save_steps=None,
                                 num_epochs=1, gradient_accumulation_steps=1, output_path=str(tmp_path), remove_prefix_in_ckpt="pipe.dit.",
                                 control_signal_type="canny_edge", num_frames=5, max_grad_norm=cfg["max_grad_norm"], controlnet_checkpoint=None)
    control = torch.zeros(5, 480, 832, 3, dtype=torch.uint8)
    items = [dict(video=[], control_video=control, file_id=str(i)) for i in range(cfg["steps"])]
    training.ModelLogger.on_step_end = spy_end
    try:
        training.launch_training_task(items, pipe, args=args, forward=forward, shuffle=False, now=datetime.datetime(2026, 1, 2, 3, 4, 5))
    finally:
        training.ModelLogger.on_step_end = real_end
    assert rec["lr"] == [float(v) for v in g["lr"]], (rec["lr"], g["lr"])
    lf, lb, nf, nb = g["loss_f32"], g["loss_bf16"], g["grad_norm_f32"], g["grad_norm_bf16"]
    print(f"PIN g22: losses {[round(v, 5) for v in rec['loss']]} (fp32 {[round(float(v), 5) for v in lf]}); gradient norms "
          f"{[round(v, 5) for v in rec['norm']]} (fp32 {[round(float(v), 5) for v in nf]})")
    for k in range(cfg["steps"]):
        assert abs(rec["loss"][k] - lf[k]) <= 2 * abs(lb[k] - lf[k]) + 2e-2 * abs(lf[k]), (k, rec["loss"][k], lf[k], lb[k])
        assert abs(rec["norm"][k] - nf[k]) <= 2 * abs(nb[k] - nf[k]) + 5e-2 * nf[k], (k, rec["norm"][k], nf[k], nb[k])
