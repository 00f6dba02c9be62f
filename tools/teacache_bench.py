#!/usr/bin/env python3
"""What a TeaCache-skipped step saves and what carrying the cache costs, at production size (A14B dimensions, 21 x 30 x 52 = 32760
tokens, ControlNet on; random-init weights as in bench.py, which is not to be touched and has no TeaCache leg).

    python tools/teacache_bench.py OUTDIR [--reps 3] [--rounds 3] [--skipped 0:0,5:5,10:14] [--parent-tree DIR]

1. Forward times (device events, `--reps` each, alternating): a computed and a skipped forward of each expert through
   model_fn_wan_video.  The decisions are FORCED through a stub object that replays a fixed pattern: a random-init time embedding is
   chaotic from step to step (on this project's tiny seeded model the reference measures relative L1 distances around 0.9 per step;
   trained checkpoints give a few percent), so random weights never skip.  How many steps a trained A14B checkpoint skips at a given
   threshold is NOT measured here and is an INPUT of this tool (`--skipped high:low,...`), not a result.
2. Derived frames/s of the 50-step loop (21 high-noise + 29 low-noise steps, denoise only) for each `--skipped` pair: a computed step
   costs the step time measured in 3 (TeaCache off), a skipped step two skipped forwards (the CFG/Euler update, ~20 us, is left out).
3. The cost of carrying the cache on a computed step (one copy of x, one subtraction, one 8-byte read-back per forward): the time of
   four steps (ids 4, 5, 30, 31) with `tea_cache_l1_thresh=0.0` (nothing skips — checked) against TeaCache off and, with
   `--parent-tree` (a checkout of the parent commit with its library built), against that commit's own package on its own modules,
   `--rounds` alternating rounds in this one process.  Passes if the median difference lies inside the min-to-max spread of the
   baseline's own repeats (the parent's if given, else the off runs'); both numbers are recorded.

Prints one JSON line and writes it to OUTDIR/teacache_bench.json.
"""
import argparse
import importlib
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LATENT = (1, 16, 21, 60, 104)
STEP_IDS = [4, 5, 30, 31]           # two high-noise and two low-noise steps of the 50-step schedule


class Replay:
    """The three calls of model_fn_wan_video with the decisions read from a list."""

    def __init__(self, ops, pattern):
        self.ops, self.pattern, self.kept, self.residual = ops, list(pattern), None, None

    def check(self, dit, x, t_mod):
        skip = self.pattern.pop(0)
        if not skip:
            self.kept = x.clone()
        return skip

    def store(self, x):
        self.residual, self.kept = self.ops.sub(x, self.kept, out=self.kept), None

    def update(self, x):
        return self.ops.add(x, self.residual)


def load_package(tree, name):
    """The goal_force_amd package of another checkout under another module name (its own _lib, ops and library)."""
    d = os.path.join(tree, "goal_force_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return name


def build(pkg, layers, dev):
    P, D = importlib.import_module(pkg + ".pipeline"), importlib.import_module(pkg + ".dit")
    cfg = dict(D.A14B_CONFIG)
    cfg["num_layers"] = layers
    n_cn = min(10, layers)
    return P.WanVideoPipeline.from_modules(
        P.build_random_expert(cfg, seed=100, device=dev), P.build_random_expert(cfg, seed=200, device=dev),
        P.build_random_controlnet(n_cn, cfg, seed=300, device=dev),
        P.build_random_controlnet(n_cn, cfg, seed=400, device=dev, zero_convs_zero=True), vae=None, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skipped", default="0:0,5:5,10:10,10:14", help="high:low numbers of skipped steps for the derived table")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--layers", type=int, default=40, help=argparse.SUPPRESS)       # debugging only; 40 = the real model
    args = ap.parse_args()
    skipped = [tuple(int(v) for v in pair.split(":")) for pair in args.skipped.split(",")]
    if any(not (0 <= h <= 20 and 0 <= l <= 28) for h, l in skipped):        # the first and the last step of the loop always compute
        raise SystemExit("--skipped: at most 20 of the 21 high-noise and 28 of the 29 low-noise steps can skip")
    os.makedirs(args.outdir, exist_ok=True)

    import torch
    from goal_force_amd import ops, teacache
    from goal_force_amd.model_fn import ContextCache, model_fn_wan_video
    if not torch.cuda.is_available():
        raise SystemExit("teacache_bench.py measures on the GPU; there is no CPU path")
    torch.set_grad_enabled(False)
    dev = torch.device("cuda", 0)
    bf = torch.bfloat16
    pipe = build("goal_force_amd", args.layers, dev)
    variants = {"off": (pipe, None), "thresh0": (pipe, 0.0)}
    if args.parent_tree:
        variants = {"parent": (build(load_package(args.parent_tree, "goal_force_amd_parent"), args.layers, dev), None), **variants}
    g = torch.Generator().manual_seed(1000)
    latents = torch.randn(LATENT, generator=torch.Generator().manual_seed(0)).to(bf).to(dev)
    y = torch.randn((1, 20) + LATENT[2:], generator=g)
    y[:, :4] = 0
    y[:, :4, 0] = 1
    y = y.to(bf).to(dev)
    control = torch.randn(LATENT, generator=g).to(bf).to(dev)
    ctx_p, ctx_n = torch.randn((1, 512, 4096), generator=g), torch.randn((1, 512, 4096), generator=g)
    ctx_p[:, 40:] = 0
    ctx_n[:, 40:] = 0
    ctx_p, ctx_n = ctx_p.to(bf).to(dev), ctx_n.to(bf).to(dev)

    # ---- 1. forwards
    pipe.scheduler.set_timesteps(50, denoising_strength=1.0, shift=5.0)
    forwards = {}
    for name, dit, cn, step in (("high_noise", pipe.dit, pipe.controlnet, 5), ("low_noise", pipe.dit2, pipe.controlnet2, 30)):
        ts = pipe.scheduler.timesteps[step].unsqueeze(0).to(dtype=bf, device=dev)
        pattern = [False] + [False, True] * args.reps                    # one warm-up (it stores the residual), then alternating
        stub, cc, ev = Replay(ops, pattern), ContextCache(), []
        for skip in pattern:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model_fn_wan_video(dit=dit, controlnet=cn, latents=latents, timestep=ts, context=ctx_p, y=y,
                               control_signal_video_latents=control, context_cache=cc, tea_cache=stub)
            e1.record()
            ev.append((skip, e0, e1))
        torch.cuda.synchronize()
        ms = {k: [a.elapsed_time(b) for s, a, b in ev[1:] if s == k] for k in (False, True)}
        forwards[name] = {"computed_ms": ms[False], "skipped_ms": ms[True], "computed_ms_median": statistics.median(ms[False]),
                          "skipped_ms_median": statistics.median(ms[True])}
        print(f"{name}: computed forward {forwards[name]['computed_ms_median']:.1f} ms, skipped {forwards[name]['skipped_ms_median']:.2f} ms",
              file=sys.stderr, flush=True)
        del stub

    # ---- 3. computed steps with and without the cache (and the parent commit), alternating
    n_skips, real_decide = [0], teacache.TeaCache.decide

    def counting_decide(self, ratio):
        skip = real_decide(self, ratio)
        n_skips[0] += bool(skip)
        return skip
    teacache.TeaCache.decide = counting_decide

    def steps(variant):
        p, thresh = variants[variant]
        kw = {} if thresh is None else {"tea_cache_l1_thresh": thresh, "tea_cache_model_id": "Wan2.1-I2V-14B-480P"}
        p.denoise(latents, ctx_p, ctx_n, y, control, num_inference_steps=50, cfg_scale=5.0, controlnet=True, step_ids=STEP_IDS,
                  record_step_times=True, **kw)
        return list(p.last_step_ms)
    rounds = {v: [] for v in variants}
    try:
        for v in variants:
            steps(v)                                                     # warm-up: context caches are per call, code objects are not
        for _ in range(args.rounds):
            for v in variants:
                rounds[v].append(steps(v))
    finally:
        teacache.TeaCache.decide = real_decide
    if n_skips[0]:
        raise SystemExit(f"tea_cache_l1_thresh=0.0 skipped {n_skips[0]} forwards: the comparison is not one of computed steps")
    total = {v: [sum(ms for ms, _ in r) for r in rs] for v, rs in rounds.items()}
    base = "parent" if "parent" in variants else "off"
    spread = max(total[base]) - min(total[base])
    overhead = {"step_ids": STEP_IDS, "rounds": args.rounds, "ms_of_4_steps": total, "median_ms": {v: statistics.median(t) for v, t in total.items()},
                "baseline": base, "baseline_spread_ms": spread,
                "thresh0_minus_off_ms": statistics.median(total["thresh0"]) - statistics.median(total["off"]),
                "thresh0_minus_baseline_ms": statistics.median(total["thresh0"]) - statistics.median(total[base]),
                "off_minus_baseline_ms": statistics.median(total["off"]) - statistics.median(total[base])}
    overhead["inside_baseline_spread"] = bool(abs(overhead["thresh0_minus_baseline_ms"]) <= spread and abs(overhead["off_minus_baseline_ms"]) <= spread)

    # ---- 2. the loop, derived
    hi = statistics.median(ms for r in rounds["off"] for ms, low in r if not low)
    lo = statistics.median(ms for r in rounds["off"] for ms, low in r if low)
    hi_s, lo_s = 2 * forwards["high_noise"]["skipped_ms_median"], 2 * forwards["low_noise"]["skipped_ms_median"]
    table = []
    for kh, kl in skipped:
        loop = ((21 - kh) * hi + kh * hi_s + (29 - kl) * lo + kl * lo_s) / 1e3
        table.append({"skipped_high_noise": kh, "skipped_low_noise": kl, "denoise_loop_s": loop, "frames_per_sec_denoise_only": 81.0 / loop})
    out = {"tool": "teacache_bench", "device": torch.cuda.get_device_name(0), "tokens": 21 * 30 * 52, "layers": args.layers, "reps": args.reps,
           "forwards": forwards, "computed_step_ms": {"high_noise": hi, "low_noise": lo},
           "skipped_step_ms": {"high_noise": hi_s, "low_noise": lo_s, "definition": "two skipped forwards"},
           "loop": table, "loop_note": "skip counts are inputs (forced), not measured on a trained checkpoint",
           "carrying_cost": overhead}
    line = json.dumps(out)
    with open(os.path.join(args.outdir, "teacache_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
