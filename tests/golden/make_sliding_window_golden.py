"""Generates tests/golden/g20_sliding_window.npz by RUNNING THE REFERENCE's own sliding-window sampling (build container only, like
make_goldens.py, whose helpers build the models):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sliding_window_golden.py

(a) tiler cases — the reference's `TemporalTiler_BCTHW().run` (GF:1296-1345) around sliding_window_refs.toy_model_fn in bf16 for every
    (T, size, stride) of sliding_window_refs.TILER_CASES: the inputs, every window's output (concatenated along T in schedule order) and
    `value`.
(b) the reference's `model_fn_wan_video` (GF:1381-1405) on the tiny expert of g5 with controlnet=None and a sliding window, for
    sliding_window_refs.MODEL_FN_CASES, in bf16 and fp32.
(c) the reference's `WanVideoPipeline.__call__` on the tiny experts of g13, built without ControlNets, with
    sliding_window_refs.PIPELINE_KWARGS (17 frames = 5 latent frames, 3 steps, window (3, 2)), in bf16 and fp32: the final latents and
    the list of window forwards (expert 2?, t, t_, timestep).

The run ASSERTS that the reference's windowed forward does not see the ControlNet: with `controlnet=cn` and the control latents it
returns the bits it returns with `controlnet=None` (its window keywords, GF:1382-1397, carry neither).  That is the evidence for the
one place where the product departs from it (goal_force_amd/model_fn.py): there the ControlNet follows its window."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_goldens as mg  # noqa: E402  (imports _ref_import, disables grad)
import gen_inputs as gi  # noqa: E402
import sliding_window_refs as sw  # noqa: E402

BF = torch.bfloat16


def tiler_cases(G, out):
    for T, size, stride in sw.TILER_CASES:
        latents, y = sw.tiler_inputs(T)
        outs = []

        def spy(**kw):
            outs.append(sw.toy_model_fn(**kw))
            return outs[-1]
        kwargs = dict(latents=latents, y=y)
        value = G.TemporalTiler_BCTHW().run(spy, size, stride, "cpu", BF, model_kwargs=kwargs, tensor_names=["latents", "y"])
        assert value.dtype == BF and tuple(value.shape) == tuple(latents.shape) and bool(torch.isfinite(value.float()).all())
        assert [o.shape[2] for o in outs] == [t_ - t for t, t_ in sw.windows(T, size, stride)], "the restated schedule is not the reference's"
        k = sw.case_key(T, size, stride)
        out[f"a_{k}_latents"], out[f"a_{k}_y"] = gi.to_u16(latents), gi.to_u16(y)
        out[f"a_{k}_windows"] = gi.to_u16(torch.cat(outs, dim=2))
        out[f"a_{k}_value"] = gi.to_u16(value)
        print("tiler", k, "windows", sw.windows(T, size, stride), flush=True)


def model_fn_cases(ref, out):
    G = ref.gf
    for mode, dt in (("bf16", BF), ("f32", torch.float32)):
        st = (lambda t: gi.to_u16(t)) if dt == BF else (lambda t: t.numpy())
        dit, cn, dsd, csd = mg._build_tiny_models(ref, False, dt)
        out["ck_dit"], out["ck_controlnet"] = np.array(gi.checksum(dsd)), np.array(gi.checksum(csd))
        ts = torch.tensor([sw.MODEL_FN_TIMESTEP], dtype=BF).to(dt)           # the timestep is rounded to bf16 first (GF:707)
        for T, size, stride in sw.MODEL_FN_CASES:
            inp = sw.model_fn_inputs(T)
            kw = dict(dit=dit, latents=inp["latents"].to(dt), timestep=ts, context=inp["ctx_posi"].to(dt), y=inp["y"].to(dt),
                      sliding_window_size=size, sliding_window_stride=stride)
            got = G.model_fn_wan_video(controlnet=None, **kw)
            with_cn = G.model_fn_wan_video(controlnet=cn, control_signal_video_latents=inp["control"].to(dt), **kw)
            assert torch.equal(got, with_cn), "the reference's windowed forward saw the ControlNet"
            dense_cn = G.model_fn_wan_video(controlnet=cn, control_signal_video_latents=inp["control"].to(dt),
                                            **{k: v for k, v in kw.items() if not k.startswith("sliding")})
            dense = G.model_fn_wan_video(controlnet=None, **{k: v for k, v in kw.items() if not k.startswith("sliding")})
            assert not torch.equal(dense, dense_cn), "this ControlNet changes nothing: the assertion above would show nothing"
            k = sw.case_key(T, size, stride)
            out[f"b_{k}_{mode}"] = st(got)
            out[f"b_{k}_ck_inputs"] = np.array(gi.checksum(inp))
            print("model_fn", mode, k, tuple(got.shape), "rms", float(got.float().pow(2).mean().sqrt()), flush=True)
    for T, size, stride in sw.MODEL_FN_CASES:
        k = sw.case_key(T, size, stride)
        a, b = gi.from_u16(out[f"b_{k}_bf16"]).float(), torch.from_numpy(out[f"b_{k}_f32"])
        print("model_fn", k, "reference bf16 vs fp32 rel-L2:", float((a - b).norm() / b.norm()), flush=True)


def pipeline_case(ref, out):
    G, _ = mg._full_reference_module()
    g6 = np.load(os.path.join(HERE, "g6_vae.npz"))
    vsd = gi.vae_decoder_sd(list(g6["names"]), g6["shapes"], seed=61)
    image, control = gi.preloop_inputs()
    inp = gi.tiny_inputs()
    kwargs = dict(sw.PIPELINE_KWARGS)
    out["c_kwargs_repr"] = np.array(repr(sorted(kwargs.items())))
    out["c_ck_inputs"] = np.array(gi.checksum([torch.from_numpy(np.array(image)).float(), inp["ctx_posi"], inp["ctx_nega"]]))
    real_fn = G.model_fn_wan_video
    for mode, dt in (("bf16", BF), ("f32", torch.float32)):
        pipe, (dit1, dit2, _, _), _, _ = mg._full_reference_pipeline(ref, G, dt, vsd, inp)
        # a pipeline built with controlnet=False: no ControlNet among the models of the loop (GF:163-168 undone)
        pipe.controlnet = pipe.controlnet2 = None
        pipe.in_iteration_models = tuple(n for n in pipe.in_iteration_models if n != "controlnet")
        pipe.in_iteration_models_2 = tuple(n for n in pipe.in_iteration_models_2 if n != "controlnet2")
        seen, calls = {}, []
        real_decode = pipe.vae.decode

        def spy_decode(hidden_states, *a, **k):
            seen["latents"] = hidden_states.detach().clone()
            return real_decode(hidden_states, *a, **k)

        def spy_fn(**kw):
            # the tiler calls the module's `model_fn_wan_video` once per window with a view of the whole latents (GF:1332): the
            # view's offset is the window's first frame
            lat = kw["latents"]
            t = lat.storage_offset() // lat.stride(2)
            calls.append((float(kw["dit"] is dit2), float(t), float(t + lat.shape[2]), float(kw["timestep"].float())))
            return real_fn(**kw)
        pipe.vae.decode = spy_decode
        G.model_fn_wan_video = spy_fn          # pipe.model_fn still is the real function: only the windows come through here
        try:
            # (the reference's control-video unit encodes `control_signal_video` whether or not a ControlNet runs, GF:798-805, and
            # fails on None: it gets 17 frames that nothing reads afterwards)
            frames = pipe(prompt=gi.PIPELINE_PROMPTS[0], negative_prompt=gi.PIPELINE_PROMPTS[1], input_image=image,
                          control_signal_video=torch.cat([control, control[:8]]).to(dt), progress_bar_cmd=lambda it: it, **kwargs)
        finally:
            G.model_fn_wan_video = real_fn
        T = (kwargs["num_frames"] - 1) // 4 + 1
        n_win = len(sw.windows(T, kwargs["sliding_window_size"], kwargs["sliding_window_stride"]))
        assert len(frames) == kwargs["num_frames"] and tuple(seen["latents"].shape) == (1, 16, T, 8, 12)
        assert len(calls) == 2 * kwargs["num_inference_steps"] * n_win, calls
        assert [c[1:3] for c in calls[:n_win]] == [tuple(map(float, w)) for w in sw.windows(T, 3, 2)], calls[:n_win]
        out[f"c_latents_{mode}"] = gi.to_u16(seen["latents"]) if dt == BF else seen["latents"].numpy()
        out[f"c_calls_{mode}"] = np.array(calls, dtype=np.float64)
        print("pipeline", mode, "calls", calls, flush=True)
    assert np.array_equal(out["c_calls_bf16"][:, :3], out["c_calls_f32"][:, :3])
    a, b = gi.from_u16(out["c_latents_bf16"]).float(), torch.from_numpy(out["c_latents_f32"])
    print("pipeline: reference bf16 vs fp32 latents rel-L2:", float((a - b).norm() / b.norm()))


def main():
    ref = mg._ref_import.load_reference()
    out = {}
    tiler_cases(ref.gf, out)
    model_fn_cases(ref, out)
    pipeline_case(ref, out)
    mg.save("g20_sliding_window.npz", **out)


if __name__ == "__main__":
    main()
