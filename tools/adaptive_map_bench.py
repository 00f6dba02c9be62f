#!/usr/bin/env python3
"""Mass-cover sparse attention at the bench shape (40 heads, S = 32760 = grid (21, 30, 52)), everything in ONE process, the variants
alternating launch by launch, each launch bracketed by events, median of --reps:
  stages  : the map build stage by stage (pooled means of q and of k, scores, selection + CSR emit) and as the one call
            (ops.block_map_from_qk), beside the dense kernel 3 and beside the LayerNorm row kernel on [S, 5120] (671 MB moved, the
            bytes the pooling pass reads: the HBM yardstick of this process) — and the coherence-gated build beside it, alternating
            in the same process: the pooling pass with the coherence accumulator, the gated selection, the gated one call.
  maps    : for tau in --taus, with and without always = FrameWindow(1, 1), ungated and with q_coherence = k_coherence in --gates, on
            three operand sets — random, random with q x 8 (peaky logits), and a clustered synthetic (the queries and keys of a frame
            share that frame's direction): density, sparse kernel time, build + sparse against dense, and the TRUE retained softmax
            mass per (row, head), 2^(lse_sparse - lse_dense).  Random rows are incoherent (rho ~ 1/n): there the gated map is dense.
  step    : one whole high-noise denoise step (CFG pair, 40 DiT + 10 ControlNet blocks, random-init A14B-size weights), dense
            against MassCover(--step-mass, FrameWindow(1, 1)) and against the same with q_coherence = k_coherence = --step-gate,
            alternating, --step-reps each, and the rel-L2 of the step's latents from the dense run's.  Random-init weights: a number about the arithmetic of a random network, NOT a quality claim (no
            checkpoint is available to measure that); near-uniform attention is also the case where a mass cover gains least.
Prints one line per measurement and a JSON summary.

    python tools/adaptive_map_bench.py [--reps 12] [--taus 0.5,0.8,0.9,0.95] [--gates 0.5,0.75] [--step-reps 3] [--step-mass 0.9]
                                        [--step-gate 0.75] [--layers 40]
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
from goal_force_amd.sparse_attention import FrameWindow, MassCover  # noqa: E402

GRID = (21, 30, 52)
S, H = GRID[0] * GRID[1] * GRID[2], 40
BF = torch.bfloat16


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def timed(variants, reps):
    """{name: [ms]} of the callables, alternating, two warm-up rounds dropped."""
    ev = {name: [] for name in variants}
    for _ in range(reps + 2):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev[name].append((e0, e1))
    torch.cuda.synchronize()
    return {name: [a.elapsed_time(b) for a, b in pairs[2:]] for name, pairs in ev.items()}


def operands(kind, g):
    q, k, v = (torch.randn(S, H * 128, generator=g, device="cuda").to(BF) for _ in range(3))
    if kind == "logits_x8":
        q = (q.float() * 8).to(BF)
    elif kind == "clustered":
        # every frame has a direction per head (norm sqrt(128)); its queries and keys carry 0.7 x that direction on top of the noise:
        # a key of the query's own frame scores 0.49 * 128 / sqrt(128) * log2(e) = 8 log2 units above the others on average
        hw = GRID[1] * GRID[2]
        d = torch.randn(GRID[0], H * 128, generator=g, device="cuda")
        d = (d.view(GRID[0], H, 128) / d.view(GRID[0], H, 128).norm(dim=-1, keepdim=True) * 128 ** 0.5).view(GRID[0], H * 128)
        frame = torch.arange(S, device="cuda") // hw
        q = (q.float() + 0.7 * d[frame]).to(BF)
        k = (k.float() + 0.7 * d[frame]).to(BF)
    return q, k, v


def stages(args, out):
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v = operands("random", g)
    o = torch.empty_like(q)
    x = torch.randn(S, H * 128, generator=g, device="cuda").to(BF)
    y = torch.empty_like(x)
    qm, km = ops.block_means(q, H, 256), ops.block_means(k, H, 64)
    sc = ops.block_map_scores(qm, km, S, S)
    (_, qc), (_, kc) = ops.block_means_coherence(q, H, 256), ops.block_means_coherence(k, H, 64)
    gate = dict(q_coherence=qc, k_coherence=kc, q_min=0.75, k_min=0.75)
    quiet = dict(q_coherence=qc, k_coherence=kc, q_min=1e-6, k_min=1e-6)          # the gate's loads and compares, nothing fires
    # the order matters to a bandwidth-bound stage (what the launch before it left in the last-level cache): the plain and the
    # coherence pooling passes each follow a LayerNorm launch on other data, and the three one-call builds follow one another
    variants = {"dense": lambda: ops.flash_attn(q, k, v, H, out=o),
                "layernorm": lambda: ops.layernorm_modulate(x, out=y),
                "means_q": lambda: ops.block_means(q, H, 256),
                "means_k": lambda: ops.block_means(k, H, 64),
                "layernorm_again": lambda: ops.layernorm_modulate(x, out=y),
                "means_coh_q": lambda: ops.block_means_coherence(q, H, 256),
                "means_coh_k": lambda: ops.block_means_coherence(k, H, 64),
                "scores": lambda: ops.block_map_scores(qm, km, S, S),
                "select": lambda: ops.block_map_select(sc, 0.9),
                "select_gated": lambda: ops.block_map_select(sc, 0.9, **gate),
                "select_quiet": lambda: ops.block_map_select(sc, 0.9, **quiet),
                "build": lambda: ops.block_map_from_qk(q, k, H, 0.9),
                "build_gated": lambda: ops.block_map_from_qk(q, k, H, 0.9, q_min=0.75, k_min=0.75),
                "build_quiet": lambda: ops.block_map_from_qk(q, k, H, 0.9, q_min=1e-6, k_min=1e-6)}
    ms = timed(variants, args.reps)
    med = {n: statistics.median(t) for n, t in ms.items()}
    nbytes = 2 * S * H * 128 * 2
    ln_rate, pool_rate = nbytes / med["layernorm"] / 1e9, nbytes / (med["means_q"] + med["means_k"]) / 1e9
    for n in variants:
        print(f"{n:15s}: {med[n]:8.3f} ms (min {min(ms[n]):.3f}, max {max(ms[n]):.3f})", flush=True)
    print(f"pooling   : {nbytes / 1e6:.0f} MB read in {med['means_q'] + med['means_k']:.3f} ms = {pool_rate:.2f} TB/s; LayerNorm row kernel, "
          f"{nbytes / 1e6:.0f} MB moved in {med['layernorm']:.3f} ms = {ln_rate:.2f} TB/s -> pooling at x{pool_rate / ln_rate:.2f} of the yardstick", flush=True)
    print(f"build     : {med['build']:.3f} ms = {100 * med['build'] / med['dense']:.2f} % of a dense launch ({med['dense']:.3f} ms)", flush=True)
    coh_ms = med["means_coh_q"] + med["means_coh_k"]
    print(f"gated     : pooling with coherence {coh_ms:.3f} ms = x{coh_ms / (med['means_q'] + med['means_k']):.3f} of the plain pooling pass "
          f"({nbytes / coh_ms / 1e9:.2f} TB/s); with thresholds of 1e-6 (the gate's loads and compares, nothing fires): selection "
          f"{med['select_quiet']:.3f} ms = x{med['select_quiet'] / med['select']:.3f}, build {med['build_quiet']:.3f} ms = "
          f"x{med['build_quiet'] / med['build']:.3f} of the ungated build; with thresholds of 0.75 (random operands: every block is gated, "
          f"every row takes the select-all path): selection {med['select_gated']:.3f} ms, build {med['build_gated']:.3f} ms = "
          f"x{med['build_gated'] / med['build']:.3f}", flush=True)
    out["stages"] = dict(ms=med, pooling_tb_s=pool_rate, layernorm_tb_s=ln_rate, build_share_of_dense=med["build"] / med["dense"], reps=args.reps)


def maps(args, out):
    taus = [float(t) for t in args.taus.split(",") if t]
    gates = [None] + [float(t) for t in args.gates.split(",") if t]
    window = FrameWindow(1, 1)(GRID)
    rows = []
    for kind in ("random", "logits_x8", "clustered"):
        g = torch.Generator(device="cuda").manual_seed(1)
        q, k, v = operands(kind, g)
        o = torch.empty_like(q)
        _, lse_d = ops.flash_attn_lse(q, k, v, H)
        cfgs = [(tau, name, a, gate) for tau in taus for name, a in (("none", None), ("window1", window)) for gate in gates]
        built = {(tau, name, gate): ops.block_map_from_qk(q, k, H, tau, always=a, q_min=gate, k_min=gate) for tau, name, a, gate in cfgs}
        _, q_coh, k_coh = ops.block_map_from_qk(q, k, H, 0.9, want_coherence=True)
        print(f"[{kind}] coherence of the query blocks: min {float(q_coh.min()):.3f} mean {float(q_coh.mean()):.3f} max {float(q_coh.max()):.3f}; "
              f"of the key tiles: min {float(k_coh.min()):.3f} mean {float(k_coh.mean()):.3f} max {float(k_coh.max()):.3f}", flush=True)
        variants = {"dense": lambda: ops.flash_attn(q, k, v, H, out=o)}
        for (tau, name, a, gate) in cfgs:
            variants[f"build/{tau}/{name}/{gate}"] = (lambda tau=tau, a=a, gate=gate: ops.block_map_from_qk(q, k, H, tau, always=a, q_min=gate,
                                                                                                              k_min=gate))
            variants[f"sparse/{tau}/{name}/{gate}"] = (lambda bm=built[tau, name, gate]: ops.flash_attn_sparse(q, k, v, H, bm, out=o))
        ms = timed(variants, args.reps)
        med = {n: statistics.median(t) for n, t in ms.items()}
        print(f"[{kind}] dense kernel 3: {med['dense']:.3f} ms", flush=True)
        for (tau, name, a, gate) in cfgs:
            bm = built[tau, name, gate]
            _, lse_s = ops.flash_attn_sparse(q, k, v, H, bm, lse=True)
            kept = torch.exp2(lse_s.double() - lse_d.double())
            b_ms, s_ms = med[f"build/{tau}/{name}/{gate}"], med[f"sparse/{tau}/{name}/{gate}"]
            row = dict(operands=kind, tau=tau, always=name, coherence_gate=gate, density=bm.density, build_ms=b_ms, sparse_ms=s_ms, dense_ms=med["dense"],
                       speedup_build_plus_sparse=med["dense"] / (b_ms + s_ms), retained_min=float(kept.min()), retained_mean=float(kept.mean()))
            rows.append(row)
            print(f"[{kind}] tau {tau:4.2f} always {name:7s} gate {str(gate):4s}: density {bm.density:.3f} | sparse {s_ms:7.3f} ms + build {b_ms:.3f} ms = "
                  f"x{row['speedup_build_plus_sparse']:.3f} of dense | true retained mass min {row['retained_min']:.4f} mean {row['retained_mean']:.4f}",
                  flush=True)
        del q, k, v, o, built, variants
    out["maps"] = rows


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
    y = y.to(BF).to(dev)
    control = torch.randn((1, 16, 21, 60, 104), generator=g).to(BF).to(dev)
    ctx_p, ctx_n = torch.randn((1, 512, 4096), generator=g), torch.randn((1, 512, 4096), generator=g)
    ctx_p[:, 40:] = 0
    ctx_n[:, 40:] = 0
    ctx_p, ctx_n = ctx_p.to(BF).to(dev), ctx_n.to(BF).to(dev)
    patterns = {"dense": None, "mass_cover": MassCover(args.step_mass, always=FrameWindow(1, 1), keep_last=True)}
    if args.step_gate > 0:
        patterns["gated"] = MassCover(args.step_mass, always=FrameWindow(1, 1), keep_last=True, q_coherence=args.step_gate,
                                      k_coherence=args.step_gate)

    def run(name, record=False):
        enable_sparse_attention(pipe, patterns[name])
        try:
            return pipe.denoise(latents, ctx_p, ctx_n, y, control, num_inference_steps=50, cfg_scale=5.0, controlnet=True,
                                step_ids=[0], record_step_times=record)
        finally:
            enable_sparse_attention(pipe, None)

    ms, lat = {name: [] for name in patterns}, {}
    for name in patterns:
        run(name)                                             # warm-up of every path
    for _ in range(args.step_reps):
        for name in patterns:
            lat[name] = run(name, record=True).float().cpu()
            ms[name].append(pipe.last_step_ms[0][0])
    dense = statistics.median(ms["dense"])
    print(f"high-noise step: dense {dense:.1f} ms {['%.1f' % t for t in ms['dense']]}", flush=True)
    out["step"] = dict(mass=args.step_mass, always="FrameWindow(1, 1)", dense_ms=ms["dense"], layers=args.layers)
    for name, mc in patterns.items():
        if mc is None:
            continue
        sp, d, density = statistics.median(ms[name]), rel_l2(lat[name], lat["dense"]), mc.last_map.density
        print(f"high-noise step: {mc!r} {sp:.1f} ms {['%.1f' % t for t in ms[name]]} | x{dense / sp:.3f} of dense; density of the last map "
              f"built {density:.3f}; latents after the step against the dense run: rel-L2 {d:.4e} (random-init weights: a number about a "
              f"random network, not a quality claim)", flush=True)
        out["step"][name] = dict(pattern=repr(mc), ms=ms[name], speedup=dense / sp, last_map_density=density, latents_rel_l2=d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--taus", default="0.5,0.8,0.9,0.95")
    ap.add_argument("--gates", default="0.5,0.75", help="coherence thresholds of the gated rows of the maps table; empty: none")
    ap.add_argument("--step-reps", type=int, default=3, help="0: kernels only")
    ap.add_argument("--step-mass", type=float, default=0.9)
    ap.add_argument("--step-gate", type=float, default=0.75, help="q_coherence = k_coherence of the gated step; 0: no gated step")
    ap.add_argument("--layers", type=int, default=40)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adaptive_map_bench.py measures on the GPU: no device found")
    torch.set_grad_enabled(False)
    out = {"tool": "adaptive_map_bench", "tokens": S, "heads": H, "grid": list(GRID), "device": torch.cuda.get_device_name(0)}
    stages(args, out)
    maps(args, out)
    if args.step_reps > 0:
        step(args, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
