#!/usr/bin/env python3
"""Block-sparse self-attention at the bench shape (40 heads, S = 32760 = grid (21, 30, 52)), everything in ONE process, the variants
alternating launch by launch, each launch bracketed by events, median of --reps:
  kernels : the dense kernel 3 (ops.flash_attn) | the sparse kernel on the full map (the price of the index reads: "full-map
            overhead") | FrameWindow(w, 1) for w in --windows.  Each window is set against density x dense x full-map overhead; what
            is left over is load imbalance (query blocks near the clip's ends select half as many tiles as those in the middle).
  step    : one whole high-noise denoise step (CFG pair, 40 DiT + 10 ControlNet blocks, random-init A14B-size weights), dense
            against FrameWindow(--step-window, 1), alternating, --step-reps each.
  drift   : (--drift-steps N, 0 = off) the latents after N CFG steps of the bench schedule, sparse against dense: rel-L2.  Random-init
            weights: a number about the arithmetic, not about video quality (no checkpoint is available to measure that).
Prints one line per measurement and a JSON summary.

    python tools/sparse_attn_bench.py [--reps 12] [--windows 1,2,3,5] [--step-reps 3] [--step-window 3] [--drift-steps 20] [--layers 40]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from goal_force_amd import ops  # noqa: E402
from goal_force_amd.sparse_attention import FrameWindow  # noqa: E402

GRID = (21, 30, 52)
S, H = GRID[0] * GRID[1] * GRID[2], 40


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def kernels(args, out):
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v = (torch.randn(S, H * 128, generator=g, device="cuda").to(torch.bfloat16) for _ in range(3))
    o = torch.empty_like(q)
    full = ops.BlockMap(torch.ones((-(-S // 256), -(-S // 64)), dtype=torch.bool), device="cuda")
    windows = [int(w) for w in args.windows.split(",") if w]
    maps = {f"window{w}": FrameWindow(w, 1)(GRID, "cuda") for w in windows}
    # (V^T is made inside both wrappers, gf_transpose_v32: the transpose, 0.7 % of the dense time, is in every timing)
    variants = {"dense": lambda: ops.flash_attn(q, k, v, H, out=o),
                "full_map": lambda: ops.flash_attn_sparse(q, k, v, H, full, out=o)}
    for name, bm in maps.items():
        variants[name] = (lambda bm=bm: ops.flash_attn_sparse(q, k, v, H, bm, out=o))
    ev = {name: [] for name in variants}
    for _ in range(args.reps + 2):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev[name].append((e0, e1))
    torch.cuda.synchronize()
    ms = {name: [a.elapsed_time(b) for a, b in pairs[2:]] for name, pairs in ev.items()}
    med = {name: statistics.median(t) for name, t in ms.items()}
    overhead = med["full_map"] / med["dense"]
    print(f"dense kernel 3      : {med['dense']:.3f} ms (min {min(ms['dense']):.3f}, max {max(ms['dense']):.3f})", flush=True)
    print(f"sparse, full map    : {med['full_map']:.3f} ms -> full-map overhead x{overhead:.4f}", flush=True)
    rows = []
    for w in windows:
        bm, t = maps[f"window{w}"], med[f"window{w}"]
        counts = bm.counts()[0]
        model = bm.density * med["dense"] * overhead
        rows.append(dict(window=w, density=bm.density, ms=t, speedup_vs_dense=med["dense"] / t, density_model_ms=model,
                         imbalance=t / model, tiles_min=int(counts.min()), tiles_max=int(counts.max())))
        print(f"FrameWindow({w}, 1)   : density {bm.density:.3f} (rows of {int(counts.min())} .. {int(counts.max())} tiles): {t:.3f} ms = x{med['dense'] / t:.2f} "
              f"of dense; density x dense x overhead = {model:.3f} ms, the rest x{t / model:.3f}", flush=True)
    out["kernels"] = dict(dense_ms=med["dense"], full_map_ms=med["full_map"], full_map_overhead=overhead, windows=rows, reps=args.reps)


def step(args, out):
    from goal_force_amd.dit import A14B_CONFIG, enable_sparse_attention
    from goal_force_amd.pipeline import WanVideoPipeline, build_random_controlnet, build_random_expert
    cfg = dict(A14B_CONFIG)
    cfg["num_layers"] = args.layers
    n_cn = min(10, args.layers)
    dev = torch.device("cuda", 0)
    pipe = WanVideoPipeline.from_modules(build_random_expert(cfg, seed=100, device=dev), build_random_expert(cfg, seed=200, device=dev),
                                         build_random_controlnet(n_cn, cfg, seed=300, device=dev),
                                         build_random_controlnet(n_cn, cfg, seed=400, device=dev, zero_convs_zero=True), device=dev)
    g = torch.Generator().manual_seed(1000)                  # bench.py's synthetic conditioning of video 0
    latents = pipe.generate_noise((1, 16, 21, 60, 104), seed=0)
    y = torch.randn((1, 20, 21, 60, 104), generator=g)
    y[:, :4] = 0
    y[:, :4, 0] = 1
    y = y.to(torch.bfloat16).to(dev)
    control = torch.randn((1, 16, 21, 60, 104), generator=g).to(torch.bfloat16).to(dev)
    ctx_p, ctx_n = torch.randn((1, 512, 4096), generator=g), torch.randn((1, 512, 4096), generator=g)
    ctx_p[:, 40:] = 0
    ctx_n[:, 40:] = 0
    ctx_p, ctx_n = ctx_p.to(torch.bfloat16).to(dev), ctx_n.to(torch.bfloat16).to(dev)
    fw = FrameWindow(args.step_window, 1)

    def run(ids, n_sched, sparse, record=False):
        enable_sparse_attention(pipe, fw if sparse else None)
        try:
            return pipe.denoise(latents, ctx_p, ctx_n, y, control, num_inference_steps=n_sched, cfg_scale=5.0, controlnet=True,
                                step_ids=ids, record_step_times=record)
        finally:
            enable_sparse_attention(pipe, None)

    ms = {False: [], True: []}
    for sparse in (False, True):
        run([0], 50, sparse)                                  # warm-up of both paths
    for _ in range(args.step_reps):
        for sparse in (False, True):
            run([0], 50, sparse, record=True)
            ms[sparse].append(pipe.last_step_ms[0][0])
    dense, sp = statistics.median(ms[False]), statistics.median(ms[True])
    print(f"high-noise step     : dense {dense:.1f} ms {['%.1f' % t for t in ms[False]]} | FrameWindow({args.step_window}, 1) {sp:.1f} ms "
          f"{['%.1f' % t for t in ms[True]]} | x{dense / sp:.3f}", flush=True)
    out["step"] = dict(window=args.step_window, density=fw(GRID).density, dense_ms=ms[False], sparse_ms=ms[True], speedup=dense / sp,
                       layers=args.layers)
    if args.drift_steps > 0:
        n = args.drift_steps
        a = run(None, n, False).float().cpu()
        b = run(None, n, True).float().cpu()
        d = rel_l2(b, a)
        print(f"drift               : latents after {n} CFG steps, FrameWindow({args.step_window}, 1) against dense, random-init weights: rel-L2 {d:.4e} "
              f"(finite: {bool(torch.isfinite(b).all())})", flush=True)
        out["drift"] = dict(steps=n, rel_l2=d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--windows", default="1,2,3,5")
    ap.add_argument("--step-reps", type=int, default=3, help="0: kernels only")
    ap.add_argument("--step-window", type=int, default=3)
    ap.add_argument("--drift-steps", type=int, default=0)
    ap.add_argument("--layers", type=int, default=40)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_attn_bench.py measures on the GPU: no device found")
    torch.set_grad_enabled(False)
    out = {"tool": "sparse_attn_bench", "tokens": S, "heads": H, "grid": list(GRID), "device": torch.cuda.get_device_name(0)}
    kernels(args, out)
    if args.step_reps > 0:
        step(args, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
