"""Sliding-window sampling at production size (profiles/r21/README.md): one process, a random-init A14B expert with its 10-block
ControlNet, 480 x 832, the high-noise step of the 50-step schedule (CFG 5: two forwards + the Euler update), timed with device events
after one warm-up per configuration, configurations alternating over the rounds:

  * 161 frames (T = 41 latent frames) with windows (21, 10) — three windows — and (21, 20) — two windows;
  * 81 frames (T = 21), the shape the kernels were tuned at, for "window count x the 81-frame step";
  * the gf_window_blend launches of one forward plus gf_window_finalize alone, at [16, 41, 60, 104];
  * the dense one-pass step at T = 41 (S = 63 960 tokens), last, with --dense.

    python tools/sliding_window_bench.py [--rounds 2] [--dense] [--layers 40]

Prints one JSON line.  Random weights: the numbers are times; what windows do to a trained model's videos is not measured here."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--dense", action="store_true", help="also time the dense one-pass step at T = 41")
    ap.add_argument("--layers", type=int, default=40)
    args = ap.parse_args()
    import torch
    from goal_force_amd import ops
    from goal_force_amd.dit import A14B_CONFIG
    from goal_force_amd.pipeline import WanVideoPipeline, build_random_controlnet, build_random_expert
    from goal_force_amd.temporal_tiler import TemporalTiler_BCTHW
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    cfg = dict(A14B_CONFIG)
    cfg["num_layers"] = args.layers
    pipe = WanVideoPipeline.from_modules(build_random_expert(cfg, seed=100, device=dev), None,
                                         build_random_controlnet(min(10, args.layers), cfg, seed=300, device=dev), None, device=dev)
    g = torch.Generator().manual_seed(1000)

    def inputs(T):
        y = torch.randn((1, 20, T, 60, 104), generator=g)
        y[:, :4] = 0
        y[:, :4, 0] = 1
        return dict(latents=pipe.generate_noise((1, 16, T, 60, 104), seed=0), y=y.to(torch.bfloat16).to(dev),
                    control=torch.randn((1, 16, T, 60, 104), generator=g).to(torch.bfloat16).to(dev))
    ctx = [torch.randn((1, 512, 4096), generator=g) for _ in range(2)]
    for c in ctx:
        c[:, 40:] = 0
    ctx = [c.to(torch.bfloat16).to(dev) for c in ctx]
    short, long = inputs(21), inputs(41)

    def step(inp, **win):
        lat = pipe.denoise(inp["latents"], ctx[0], ctx[1], inp["y"], inp["control"], num_inference_steps=50, cfg_scale=5.0,
                           controlnet=True, step_ids=[0], record_step_times=True, **win)
        assert bool(torch.isfinite(lat.float()).all())
        return pipe.last_step_ms[0][0]

    configs = {"T21_dense": lambda: step(short), "T41_window_21_10": lambda: step(long, sliding_window_size=21, sliding_window_stride=10),
               "T41_window_21_20": lambda: step(long, sliding_window_size=21, sliding_window_stride=20)}
    times = {k: [] for k in configs}
    for rnd in range(args.rounds + 1):                    # round 0 warms every shape up
        for name, run in configs.items():
            ms = run()
            if rnd:
                times[name].append(ms)
            print(f"round {rnd} {name}: {ms:.1f} ms", file=sys.stderr, flush=True)

    # the blend launches of ONE windowed forward at T = 41 and the final division, alone
    blend = {}
    for size, stride in ((21, 10), (21, 20)):
        wins = TemporalTiler_BCTHW.windows(41, size, stride)
        outs = [torch.randn((1, 16, t_ - t, 60, 104), device=dev).to(torch.bfloat16) for t, t_ in wins]
        value, weight = torch.zeros((1, 16, 41, 60, 104), dtype=torch.bfloat16, device=dev), torch.zeros((41,), dtype=torch.bfloat16, device=dev)

        def once():
            value.zero_()
            weight.zero_()
            for (t, t_), o in zip(wins, outs):
                ops.window_blend(value, weight, o, t, (t == 0, t_ == 41), size - stride)
            ops.window_finalize(value, weight)
        for _ in range(3):
            once()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(50):
            once()
        ev[1].record()
        torch.cuda.synchronize()
        blend[f"window_{size}_{stride}"] = ev[0].elapsed_time(ev[1]) / 50
    out = {"device": torch.cuda.get_device_name(0), "layers": args.layers, "rounds": args.rounds, "step_ms": times,
           "windows": {"21_10": len(TemporalTiler_BCTHW.windows(41, 21, 10)), "21_20": len(TemporalTiler_BCTHW.windows(41, 21, 20))},
           "blend_ms_per_forward_incl_zeroing": blend}
    print(json.dumps(out), flush=True)
    if args.dense:
        dense = []
        for rnd in range(2):
            ms = step(long)
            if rnd:
                dense.append(ms)
            print(f"round {rnd} T41_dense: {ms:.1f} ms", file=sys.stderr, flush=True)
        print(json.dumps({"step_ms": {"T41_dense": dense}}), flush=True)


if __name__ == "__main__":
    main()
