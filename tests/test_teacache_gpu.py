"""TeaCache on the GPU: the two kernels, the three calls inside model_fn_wan_video, and `pipe(..., tea_cache_l1_thresh=,
tea_cache_model_id=)` end to end against what the REFERENCE's own `WanVideoPipeline.__call__` decided and produced for the same
arguments (tests/golden/g19_teacache.npz, tests/golden/make_teacache_golden.py; inputs in tests/teacache_inputs.py)."""
import os
import types

import numpy as np
import pytest
import torch

import gen_inputs as gi
import teacache_inputs as ti
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


# ------------------------------------------------------------------ kernels
def _tmod_pair(n, kind, seed):
    g = torch.Generator().manual_seed(seed)
    prev = (3.0 * torch.randn(n, generator=g)).to(BF)
    if kind == "random":
        cur = (3.0 * torch.randn(n, generator=g)).to(BF)
    else:                                                   # consecutive steps of a trained projection: 2 % apart
        cur = (prev.float() * (1 + 0.02 * torch.randn(n, generator=g))).to(BF)
    return cur, prev


@pytest.mark.parametrize("kind", ["random", "perturbed"])
@pytest.mark.parametrize("n", [1536, 30720])
def test_rel_l1_sums(n, kind):
    """Both sums within 1e-5 relative of fp64 sums of the same bf16-rounded terms (an fp32 tree sum of 30720 non-negative terms is
    good to about log2(n) * 2^-24 ~ 1e-6: a tenfold margin), and the same bits on a second call (fixed-order reduction, no atomics)."""
    from goal_force_amd import ops
    cur, prev = _tmod_pair(n, kind, seed=n + len(kind))
    want_d = float((cur - prev).abs().double().sum())       # torch's CPU bf16 subtraction rounds the fp32 difference once per element
    want_p = float(prev.abs().double().sum())
    c, p = cur.cuda().view(6, -1), prev.cuda().view(6, -1)
    got = ops.rel_l1(c, p)
    again = ops.rel_l1(c, p)
    print(f"rel_l1 n={n} {kind}: diff {got[0]!r} (fp64 {want_d!r}), prev {got[1]!r} (fp64 {want_p!r})")
    assert isinstance(got[0], float) and isinstance(got[1], float)
    assert abs(got[0] - want_d) <= 1e-5 * want_d and abs(got[1] - want_p) <= 1e-5 * want_p
    assert np.float32(got[0]).tobytes() == np.float32(again[0]).tobytes() and np.float32(got[1]).tobytes() == np.float32(again[1]).tobytes()


@pytest.mark.parametrize("shape", [(72, 256), (33, 5120), (5, 3)])
def test_sub_is_torch_bf16_subtraction(shape):
    """Bit-equal to torch's bf16 `a - b` on the CPU; [33, 5120] is more than one block with a ragged last one, [5, 3] is all tail;
    `out` aliasing `a`."""
    from goal_force_amd import ops
    g = torch.Generator().manual_seed(sum(shape))
    a, b = torch.randn(shape, generator=g).to(BF), (torch.randn(shape, generator=g) * 0.9).to(BF)
    b[0, :2] = a[0, :2]                                     # exact zeros
    want = a - b
    da, db = a.cuda(), b.cuda()
    assert torch.equal(ops.sub(da, db).cpu(), want)
    assert torch.equal(da.cpu(), a)
    out = ops.sub(da, db, out=da)
    assert out is da and torch.equal(da.cpu(), want)


def test_ops_refuse_cpu_tensors_and_ragged_sizes():
    from goal_force_amd import ops
    from goal_force_amd._lib import GoalForceError
    a = torch.zeros(16, dtype=BF)
    with pytest.raises(GoalForceError, match="must be on the GPU"):
        ops.sub(a, a)
    with pytest.raises(GoalForceError, match="must be on the GPU"):
        ops.rel_l1(a, a)
    with pytest.raises(GoalForceError, match="multiple of 8"):
        ops.rel_l1(a.cuda()[:12].contiguous(), a.cuda()[:12].contiguous())
    with pytest.raises(GoalForceError, match="equal-sized"):
        ops.sub(a.cuda(), a.cuda()[:8])
    with pytest.raises(GoalForceError, match="dtype"):
        ops.rel_l1(a.cuda().float(), a.cuda().float())


# ------------------------------------------------------------------ the models of g19
class FixedPrompter:
    """What the golden run used in place of WanPrompter (as in g13): `encode_prompt` with the reference's signature."""

    def __init__(self, inp):
        self.inp = inp

    def encode_prompt(self, prompt, positive=True, device="cuda"):
        return (self.inp["ctx_posi"] if prompt == gi.PIPELINE_PROMPTS[0] else self.inp["ctx_nega"]).to(device)


@pytest.fixture(scope="module")
def setup():
    from goal_force_amd.controlnet import ControlNet
    from goal_force_amd.dit import WanModel
    from goal_force_amd.pipeline import WanVideoPipeline
    from goal_force_amd.vae import WanVideoVAE
    g = np.load(os.path.join(GOLDEN, "g19_teacache.npz"))
    cfg = gi.TINY

    def expert(e):
        sd = ti.expert_sd(e)
        assert gi.same_checksum(gi.checksum({k: v.to(BF) for k, v in sd.items()}), g["ck_dit"][e])
        m = WanModel(has_image_input=False, require_clip_embedding=False, **cfg)
        m.load_state_dict(sd, strict=True)
        return m.to(BF).cuda()

    def cnet(zero):
        cn = ControlNet(gi.TINY_CONTROLNET_LAYERS, dim=cfg["dim"], num_heads=cfg["num_heads"], ffn_dim=cfg["ffn_dim"])
        cn.load_state_dict(gi.controlnet_sd(cfg, gi.TINY_CONTROLNET_LAYERS, seed=42, zero_convs_zero=zero), strict=True)
        return cn.to(BF).cuda()

    assert gi.same_checksum(gi.checksum(gi.controlnet_sd(cfg, gi.TINY_CONTROLNET_LAYERS, seed=42)), g["ck_controlnet"])
    g6 = np.load(os.path.join(GOLDEN, "g6_vae.npz"))
    vsd = gi.vae_decoder_sd(list(g6["names"]), g6["shapes"], seed=61)
    vae = WanVideoVAE()
    vae.load_state_dict({"model." + k: t for k, t in vsd.items()}, strict=True)
    pipe = WanVideoPipeline.from_modules(expert(0), expert(1), cnet(False), cnet(True), vae=vae.to(BF).cuda())
    image, control = gi.preloop_inputs()
    inp = gi.tiny_inputs()
    assert gi.same_checksum(gi.checksum([torch.from_numpy(np.array(image)).float(), control, inp["ctx_posi"], inp["ctx_nega"]]), g["ck_inputs"])
    assert str(g["kwargs_repr"]) == repr(sorted(ti.CALL_KWARGS.items())), "the golden was made with these keyword arguments"
    pipe.prompter = FixedPrompter(inp)
    return types.SimpleNamespace(g=g, pipe=pipe, image=image, control=control, inp=inp)


def _call(s, **over):
    kw = dict(ti.CALL_KWARGS, output_type="latent")
    kw.update(over)
    return s.pipe(prompt=gi.PIPELINE_PROMPTS[0], negative_prompt=gi.PIPELINE_PROMPTS[1], input_image=s.image,
                  control_signal_video=s.control, **kw)


def _log_decisions(monkeypatch):
    """Every `TeaCache.decide` of the product's class -> (object, ratio, accumulated distance after, skip), in call order."""
    from goal_force_amd.teacache import TeaCache
    log, real = [], TeaCache.decide

    def spy(self, ratio):
        skip = real(self, ratio)
        log.append((id(self), float("nan") if ratio is None else ratio, float(self.accumulated_rel_l1_distance), skip))
        return skip
    monkeypatch.setattr(TeaCache, "decide", spy)
    return log


def test_pipeline_call_decides_and_computes_like_the_reference_call(setup, monkeypatch):
    """`pipe(..., num_inference_steps=20, tea_cache_l1_thresh=0.26, tea_cache_model_id="Wan2.1-I2V-14B-480P")` against the reference's
    own `__call__` with exactly these arguments: the decision of every one of the 40 forwards, the `model_fn` call list (as g13's
    test), and the final latents at g13's bar — no further from the reference's fp32 run than 1.25 x the reference's own bf16 run
    (+ 1e-3), and within 2 x that of the bf16 run itself."""
    s, g = setup, setup.g
    log = _log_decisions(monkeypatch)
    calls, real_fn = [], s.pipe.model_fn

    def spy(**kw):
        calls.append((float(kw["dit"] is s.pipe.dit2), float(kw.get("controlnet") is s.pipe.controlnet2), float(kw["timestep"].float())))
        return real_fn(**kw)
    s.pipe.model_fn = spy
    try:
        lat = _call(s).float().cpu()
    finally:
        s.pipe.model_fn = real_fn
    assert calls == [tuple(r) for r in g["model_fn_calls_bf16"].tolist()]
    objs = list(dict.fromkeys(o for o, *_ in log))
    assert len(objs) == 2 and len(log) == 40                # one object per CFG branch, shared by both experts
    ratio_dev = acc_dev = 0.0
    for b, o in enumerate(objs):
        mine = [r for r in log if r[0] == o]
        assert [r[3] for r in mine] == [bool(v) for v in g["skip_bf16"][b]], f"branch {b}"
        for (_, ratio, acc, _), r_ref, a_ref in zip(mine, g["ratio_bf16"][b], g["acc_bf16"][b]):
            assert np.isnan(ratio) == np.isnan(r_ref)
            if not np.isnan(r_ref):
                ratio_dev = max(ratio_dev, abs(ratio - r_ref) / r_ref)
            if a_ref != 0:
                acc_dev = max(acc_dev, abs(acc - a_ref) / a_ref)
    f32, ref_bf = torch.from_numpy(g["latents_f32"]), gi.from_u16(g["latents_bf16"]).float()
    e, e_ref, e_bf = rel_l2(lat, f32), rel_l2(ref_bf, f32), rel_l2(lat, ref_bf)
    print(f"g19: {int(g['skip_bf16'][0].sum())} of 20 steps skipped per branch; largest relative deviation from the reference's accumulated "
          f"distances {acc_dev:.3e} (ratios {ratio_dev:.3e}); latents vs fp32 {e:.3e} (reference bf16 {e_ref:.3e}), vs ref-bf16 {e_bf:.3e}")
    assert tuple(lat.shape) == (1, 16, 3, 8, 12)
    assert e < 1.25 * e_ref + 1e-3 and e_bf < 2 * e_ref, f"latents vs fp32 {e:.3e}, vs ref-bf16 {e_bf:.3e} (reference bf16 vs fp32 {e_ref:.3e})"


def test_threshold_zero_skips_nothing_and_leaves_the_computed_path_alone(setup, monkeypatch):
    """With `tea_cache_l1_thresh=0.0` every step computes (the polynomial is positive over the fixture's ratios — asserted on the
    recorded ones), and the latents are BIT-identical to the same call without TeaCache: the bookkeeping (a copy, a subtraction, a
    read-back) must not touch what the blocks compute."""
    from goal_force_amd.teacache import COEFFICIENTS
    s = setup
    poly = np.poly1d(COEFFICIENTS[ti.CALL_KWARGS["tea_cache_model_id"]])
    ratios = s.g["ratio_bf16"][~np.isnan(s.g["ratio_bf16"])]
    assert ratios.size == 36 and np.all(poly(ratios) > 0)
    log = _log_decisions(monkeypatch)
    cached = _call(s, tea_cache_l1_thresh=0.0)
    assert len(log) == 40 and not any(r[3] for r in log)
    del log[:]
    plain = _call(s, tea_cache_l1_thresh=None)
    assert not log                                           # off: no object at all
    assert torch.equal(cached, plain)


def _forward_kw(s, step, n_steps=20):
    """One cond forward of the high-noise expert at step `step` of an n_steps schedule, on the tiny inputs of g5."""
    s.pipe.scheduler.set_timesteps(n_steps, denoising_strength=1.0, shift=5.0)
    ts = s.pipe.scheduler.timesteps[step].unsqueeze(0).to(dtype=BF, device="cuda")
    dev = {k: v.cuda() for k, v in s.inp.items()}
    return dict(dit=s.pipe.dit, controlnet=s.pipe.controlnet, latents=dev["latents"], timestep=ts, context=dev["ctx_posi"], y=dev["y"],
                control_signal_video_latents=dev["control"])


def test_skipped_forward_runs_no_block_and_is_head_of_x_plus_residual(setup):
    """Forward hooks on every DiT and ControlNet block: all fire on a computed forward, none on a skipped one (the ControlNet is
    not run and thrown away as in the reference), the `cfg_shared` memo of a skipped forward stays empty, and the skipped forward's
    output is head(patchified x + stored residual), rebuilt here from `ops` calls, bit for bit."""
    from goal_force_amd import ops
    from goal_force_amd.model_fn import model_fn_wan_video
    from goal_force_amd.teacache import TeaCache
    s = setup
    dit, cn = s.pipe.dit, s.pipe.controlnet
    blocks = list(dit.blocks) + list(cn.controlnet_dit.blocks)
    fired, last = [], {}
    hooks = [b.register_forward_hook(lambda m, a, out: fired.append(m)) for b in blocks]
    hooks.append(dit.blocks[-1].register_forward_hook(lambda m, a, out: last.__setitem__("x", out.clone())))
    try:
        tc = TeaCache(4, rel_l1_thresh=1e30, model_id="Wan2.1-I2V-14B-480P")       # steps 1 and 2 of 4 skip whatever the ratio
        memo = {}
        model_fn_wan_video(**_forward_kw(s, 0), tea_cache=tc, cfg_shared=memo)
        assert set(fired) == set(blocks) and len(fired) == len(blocks) and memo
        # store: bf16(x after the last block - patchified x); ControlNet block 0 injects before DiT block 1, so `last` is the final x
        kw = _forward_kw(s, 0)
        x0 = dit.patchify(kw["latents"], extra=kw["y"])[0][0]
        assert torch.equal(tc.previous_residual.cpu(), last["x"].cpu().view_as(x0) - x0.cpu()) and tc.previous_hidden_states is None
        for step in (1, 2):
            del fired[:]
            memo = {}
            kw = _forward_kw(s, step)
            got = model_fn_wan_video(**kw, tea_cache=tc, cfg_shared=memo)
            assert not fired and not memo, f"step {step}: a block ran on a skipped forward"
            x, grid = dit.patchify(kw["latents"], extra=kw["y"])
            t, _ = dit.time_embed(kw["timestep"])
            want = dit.unpatchify(dit.head(ops.add(x[0], tc.previous_residual).unsqueeze(0), t), grid)
            assert torch.equal(got, want)
        del fired[:]
        model_fn_wan_video(**_forward_kw(s, 3), tea_cache=tc)                        # the last step always computes
        assert set(fired) == set(blocks) and tc.step == 0
    finally:
        for h in hooks:
            h.remove()


class TorchTeaCache:
    """A caller's own plug: the three methods on plain torch ops (written from the behaviour DESIGN §4.11 states)."""

    def __init__(self, num_inference_steps, rel_l1_thresh, coefficients):
        self.n, self.thresh, self.poly = num_inference_steps, rel_l1_thresh, np.poly1d(coefficients)
        self.i, self.acc, self.prev, self.kept, self.residual, self.decisions = 0, 0.0, None, None, None, []

    def check(self, dit, x, t_mod):
        if self.i in (0, self.n - 1):
            compute, self.acc = True, 0.0
        else:
            self.acc += self.poly(((t_mod - self.prev).abs().mean() / self.prev.abs().mean()).item())
            compute = not self.acc < self.thresh
            if compute:
                self.acc = 0.0
        self.prev, self.i = t_mod.clone(), (self.i + 1) % self.n
        if compute:
            self.kept = x.clone()
        self.decisions.append(not compute)
        return not compute

    def store(self, x):
        self.residual, self.kept = x - self.kept, None

    def update(self, x):
        return x + self.residual


def test_model_fn_takes_a_duck_typed_cache(setup, monkeypatch):
    """model_fn_wan_video talks to `tea_cache` through check / store / update only: an object of the caller's that implements them
    with torch ops gives the decisions of the product's class and outputs within 1 bf16 ulp of it (first 8 steps of the g19 schedule)."""
    from goal_force_amd.model_fn import model_fn_wan_video
    from goal_force_amd.teacache import COEFFICIENTS, TeaCache
    s = setup
    log = _log_decisions(monkeypatch)
    mid, thresh = ti.CALL_KWARGS["tea_cache_model_id"], ti.CALL_KWARGS["tea_cache_l1_thresh"]
    own, plug = TeaCache(20, rel_l1_thresh=thresh, model_id=mid), TorchTeaCache(20, thresh, COEFFICIENTS[mid])
    for step in range(8):
        a = model_fn_wan_video(**_forward_kw(s, step), tea_cache=own).float()
        b = model_fn_wan_video(**_forward_kw(s, step), tea_cache=plug).float()
        ulp = torch.exp2(torch.floor(torch.log2(torch.maximum(a.abs(), b.abs()).clamp_min(1e-30))) - 7)
        assert bool(((a - b).abs() <= ulp).all()), f"step {step}: {float(((a - b).abs() / ulp).max())} ulp"
    assert [r[3] for r in log] == plug.decisions == [bool(v) for v in s.g["skip_bf16"][0][:8]]
    assert any(plug.decisions) and not all(plug.decisions)


def test_sequence_parallel_with_tea_cache_is_refused(setup):
    from goal_force_amd._lib import GoalForceError
    from goal_force_amd.model_fn import model_fn_wan_video
    from goal_force_amd.teacache import TeaCache
    tc = TeaCache(4, rel_l1_thresh=0.1, model_id="Wan2.1-I2V-14B-480P")
    group = types.SimpleNamespace(size=2, rank=0)           # refused before the group is used
    with pytest.raises(GoalForceError, match="tea_cache with sequence parallelism"):
        model_fn_wan_video(**_forward_kw(setup, 0), tea_cache=tc, sequence_parallel=group)
    assert tc.step == 0 and tc.previous_modulated_input is None
