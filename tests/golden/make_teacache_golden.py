"""Generates tests/golden/g19_teacache.npz by RUNNING THE REFERENCE's own `WanVideoPipeline.__call__` with TeaCache on (build
container only, like make_goldens.py, whose helpers build the pipeline):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_teacache_golden.py

The g13 call with tests/teacache_inputs.CALL_KWARGS (20 steps, tea_cache_l1_thresh=0.26, tea_cache_model_id="Wan2.1-I2V-14B-480P")
on the tiny experts of g13 whose time projection got a large constant part (teacache_inputs.smooth_time_projection), in bf16 and fp32.
Stored per dtype: for each of the 40 forwards the relative L1 distance the reference's `TeaCache.check` evaluated (NaN on the forced
steps, where it evaluates none), the accumulated distance after the check and the decision, per CFG branch; the `model_fn` call list
as g13 records it; the final latents; checksums of inputs and weights.

The run ASSERTS what makes the fixture a test of the decisions rather than of rounding luck: every accumulated distance is at least
10 % of the threshold away from the threshold, 5 to 15 of the 20 steps are skipped per branch, and the two branches and the two
dtypes decide alike.  If a change of the inputs breaks one of these, change the offset scale or the seeds — not the conditions."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_goldens as mg  # noqa: E402  (imports _ref_import, disables grad)
import gen_inputs as gi  # noqa: E402
import teacache_inputs as ti  # noqa: E402

BF = torch.bfloat16
MARGIN = 0.10


def main():
    ref = mg._ref_import.load_reference()
    G, _ = mg._full_reference_module()
    g6 = np.load(os.path.join(HERE, "g6_vae.npz"))
    vsd = gi.vae_decoder_sd(list(g6["names"]), g6["shapes"], seed=61)
    image, control = gi.preloop_inputs()
    inp = gi.tiny_inputs()
    kwargs = dict(ti.CALL_KWARGS)
    steps, thresh = kwargs["num_inference_steps"], kwargs["tea_cache_l1_thresh"]
    sds = [{k: v.to(BF) for k, v in ti.expert_sd(e).items()} for e in (0, 1)]
    out = {"ck_inputs": np.array(gi.checksum([torch.from_numpy(np.array(image)).float(), control, inp["ctx_posi"], inp["ctx_nega"]])),
           "ck_dit": np.array([gi.checksum(sd) for sd in sds]),
           "kwargs_repr": np.array(repr(sorted(kwargs.items())))}

    real_check = G.TeaCache.check
    for mode, dt in (("bf16", BF), ("f32", torch.float32)):
        pipe, (dit1, dit2, cn1, cn2), _, csd = mg._full_reference_pipeline(ref, G, dt, vsd, inp)
        for dit, sd in ((dit1, sds[0]), (dit2, sds[1])):
            dit.load_state_dict({k: v.to(dt) for k, v in sd.items()}, strict=True)
        out["ck_controlnet"] = np.array(gi.checksum(csd))
        seen, calls, log, order = {}, [], {}, []

        def spy_check(self, dit, x, t_mod):
            if id(self) not in log:
                order.append(id(self))
                log[id(self)] = []
            ratio = float("nan")
            if not (self.step == 0 or self.step == self.num_inference_steps - 1):      # the expression of the reference, on its operands
                prev = self.previous_modulated_input
                ratio = ((t_mod - prev).abs().mean() / prev.abs().mean()).cpu().item()
            skip = real_check(self, dit, x, t_mod)
            log[id(self)].append((ratio, float(self.accumulated_rel_l1_distance), float(skip)))
            return skip
        G.TeaCache.check = spy_check
        real_decode, real_fn = pipe.vae.decode, pipe.model_fn

        def spy_decode(hidden_states, *a, **k):
            seen["latents"] = hidden_states.detach().clone()
            return real_decode(hidden_states, *a, **k)

        def spy_fn(**kw):
            calls.append((kw["dit"] is dit2, kw.get("controlnet") is cn2, float(kw["timestep"].float())))
            return real_fn(**kw)
        pipe.vae.decode, pipe.model_fn = spy_decode, spy_fn
        try:
            pipe(prompt=gi.PIPELINE_PROMPTS[0], negative_prompt=gi.PIPELINE_PROMPTS[1], input_image=image,
                 control_signal_video=control.to(dt), progress_bar_cmd=lambda it: it, **kwargs)
        finally:
            G.TeaCache.check = real_check
        assert len(order) == 2 and len(calls) == 2 * steps and all(len(log[i]) == steps for i in order)
        rec = np.array([log[i] for i in order], dtype=np.float64)                  # [branch (cond, uncond), step, (ratio, acc, skip)]
        out[f"ratio_{mode}"], out[f"acc_{mode}"], out[f"skip_{mode}"] = rec[..., 0], rec[..., 1], rec[..., 2]
        out[f"model_fn_calls_{mode}"] = np.array(calls, dtype=np.float64)
        out[f"latents_{mode}"] = gi.to_u16(seen["latents"]) if dt == BF else seen["latents"].numpy()
        # the accumulated distance the decision was taken on: after a computing check it has been reset, so rebuild it
        checked = ~np.isnan(rec[..., 0])
        poly = np.poly1d(G.TeaCache(steps, thresh, kwargs["tea_cache_model_id"]).coefficients)
        decided_on = np.zeros_like(rec[..., 1])
        for b in range(2):
            acc = 0.0
            for s in range(steps):
                if checked[b, s]:
                    acc += poly(rec[b, s, 0])
                    decided_on[b, s] = acc
                    assert (acc < thresh) == bool(rec[b, s, 2])
                if not rec[b, s, 2]:
                    acc = 0.0
        out[f"decided_on_{mode}"] = decided_on
        gap = np.abs(decided_on[checked] - thresh) / thresh
        n_skip = rec[..., 2].sum(axis=1)
        print(mode, "skipped per branch", n_skip, "closest accumulated distance to the threshold: %.4f (%.1f %% of it away)"
              % (decided_on[checked][gap.argmin()], 100 * gap.min()), flush=True)
        print(mode, "ratios", np.round(rec[0, :, 0], 4), "\n", mode, "decided on", np.round(decided_on[0], 4), flush=True)
        assert gap.min() >= MARGIN, f"{mode}: an accumulated distance lies {100 * gap.min():.1f} % of the threshold from it"
        assert np.all((n_skip >= 5) & (n_skip <= 15)), n_skip
        assert np.array_equal(rec[0, :, 2], rec[1, :, 2]), "the two CFG branches decide differently"
    assert np.array_equal(out["skip_bf16"], out["skip_f32"]), "bf16 and fp32 decide differently"
    assert np.array_equal(out["model_fn_calls_bf16"][:, :2], out["model_fn_calls_f32"][:, :2])      # (the fp32 run's timesteps are not bf16-rounded)
    a, b = gi.from_u16(out["latents_bf16"]).float(), torch.from_numpy(out["latents_f32"])
    print("reference bf16 vs reference fp32 (both cached), latents rel-L2:", float((a - b).norm() / b.norm()))
    mg.save("g19_teacache.npz", **out)


if __name__ == "__main__":
    main()
