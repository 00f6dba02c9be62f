#!/usr/bin/env python3
"""LoRA adapters: what the attached form costs beside the plain layer, and the merge against the bytes it moves (profiles/r24/README.md).
Everything in ONE process, alternating.

  layer leg  M = 32760 at D->D, D->F, F->D with the epilogue the block runs there (gate + residual, GELU, gate + residual), ranks
             16 / 64 / 128: dit.linear on the plain layer (one gf_gemm_bf16 launch) against the same layer with one attached adapter
             (gf_gemm_bf16 with EPI_BIAS, gf_gemm_bf16 for t = x down^T, gf_lora_up with the caller's epilogue); the plain layer twice
             (A/A) for the run-to-run spread; gf_lora_up alone against the bytes it moves (y0, out, resid, t).
  merge leg  gf_lora_merge on [5120, 5120], [13824, 5120], [5120, 13824] at ranks 16 / 64 / 128 / 256 against one read and one write of W;
             the calls repeat on one W (which then sits in the Infinity Cache), so the per-expert sum of this leg is an extrapolation.
  expert     one pass over the 400 DISTINCT block weights of an A14B expert (28 GB, 56 GB moved) per rank, three passes: what a load
  merge leg  costs with every weight coming from HBM.
  step leg   one high-noise step of the bench configuration (A14B experts, 10-layer ControlNets, 21 x 60 x 104 latents, CFG): plain (twice:
             A/A) against q, k, v, o, ffn.0, ffn.2 of every DiT and ControlNet block attached at rank 64, alternating; then the same
             adapters merged (the parent's launches on other weights).  Random-init weights: a number, not a quality claim.
Prints one JSON line per leg; needs an MI355X (no fallback).
"""
import argparse
import contextlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S_TOKENS, DIM, FFN = 32760, 5120, 13824
SHAPES = {"D->D": (DIM, DIM, 2), "D->F": (FFN, DIM, 1), "F->D": (DIM, FFN, 2)}      # (N, K, the block's epilogue there)
BLOCK_LAYERS = tuple(f"{a}.{p}" for a in ("self_attn", "cross_attn") for p in "qkvo") + ("ffn.0", "ffn.2")


def timed(torch, fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def summary(xs):
    med = statistics.median(xs)
    return dict(median_ms=round(med, 4), min_ms=round(min(xs), 4), spread=round((max(xs) - min(xs)) / med, 4))


def alternate(torch, variants, rounds, calls):
    times = {v: [] for v in variants}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for v, fn in variants.items():
            times[v].append(timed(torch, fn, calls))
    return {v: summary(t) for v, t in times.items()}


def adapter_sd(torch, name, n, k, rank, g):
    return {f"{name}.lora_B.weight": (torch.randn((n, rank), generator=g) / k ** 0.5).to(torch.bfloat16),
            f"{name}.lora_A.weight": (torch.randn((rank, k), generator=g) / rank ** 0.5).to(torch.bfloat16)}


def layer_leg(torch, ops, rounds, calls, ranks):
    from goal_force_amd import dit, lora
    out = {}
    for name, (n, k, epi) in SHAPES.items():
        g = torch.Generator(device="cuda").manual_seed(n + k)
        x = torch.randn((S_TOKENS, k), device="cuda", generator=g).to(torch.bfloat16)
        resid = torch.randn((S_TOKENS, n), device="cuda", generator=g).to(torch.bfloat16)
        gate = torch.randn((n,), device="cuda", generator=g).to(torch.bfloat16)
        y = torch.empty((S_TOKENS, n), device="cuda", dtype=torch.bfloat16)
        kw = dict(epilogue=epi, resid=resid if epi == 2 else None, gate=gate if epi == 2 else None, out=y)
        plain = torch.nn.Linear(k, n).to(torch.bfloat16).cuda()
        variants = {"plain": lambda: dit.linear(x, plain, **kw)}
        cg = torch.Generator().manual_seed(7)
        mods = {}
        for r in ranks:
            lin = torch.nn.Linear(k, n).to(torch.bfloat16).cuda()
            lin.load_state_dict(plain.state_dict())
            host = torch.nn.ModuleDict({"o": lin})
            lora.attach(host, adapter_sd(torch, "o", n, k, r, cg), alpha=0.7, own_linears=True)     # (this tool calls dit.linear itself)
            ad = lora.adapters(lin)[0]
            mods[r] = host
            variants[f"attached_r{r}"] = (lambda lin: lambda: dit.linear(x, lin, **kw))(lin)
            t = ops.gemm(x, ad.down)
            y0 = ops.gemm(x, plain.weight, plain.bias)
            variants[f"lora_up_r{r}"] = (lambda ad, t, y0: lambda: ops.lora_up(y0, t, ad.up, 0.7, epilogue=epi, resid=kw["resid"], gate=kw["gate"], out=y))(ad, t, y0)
            variants[f"t_gemm_r{r}"] = (lambda ad: lambda: ops.gemm(x, ad.down))(ad)
        variants["plain_again"] = variants["plain"]
        res = alternate(torch, variants, rounds, calls)
        aa = abs(res["plain"]["median_ms"] - res["plain_again"]["median_ms"]) / res["plain"]["median_ms"]
        noise = max(aa, res["plain"]["spread"], res["plain_again"]["spread"])
        res["aa_plain_rel"], res["noise_rel"] = round(aa, 4), round(noise, 4)
        for r in ranks:
            rp = -(-r // 32) * 32
            res[f"attached_over_plain_r{r}"] = round(res[f"attached_r{r}"]["median_ms"] / res["plain"]["median_ms"], 4)
            nbytes = 2 * S_TOKENS * (n * (3 if epi == 2 else 2) + rp)
            res[f"lora_up_r{r}"]["tb_per_s"] = round(nbytes / res[f"lora_up_r{r}"]["median_ms"] / 1e9, 3)
        out[name] = res
        del x, resid, y, mods, variants
        torch.cuda.empty_cache()
    return out


def merge_leg(torch, ops, rounds, calls, ranks):
    out, per_expert = {}, {r: 0.0 for r in ranks}
    for name, (n, k, _) in SHAPES.items():
        g = torch.Generator(device="cuda").manual_seed(3 * n + k)
        w = (torch.randn((n, k), device="cuda", generator=g) / k ** 0.5).to(torch.bfloat16)
        variants = {}
        for r in ranks:
            up = (torch.randn((n, r), device="cuda", generator=g) / k ** 0.5).to(torch.bfloat16)
            down = (torch.randn((r, k), device="cuda", generator=g) / r ** 0.5).to(torch.bfloat16)
            variants[f"r{r}"] = (lambda up, down: lambda: ops.lora_merge(w, up, down, 1e-3))(up, down)
        res = alternate(torch, variants, rounds, calls)
        for r in ranks:
            res[f"r{r}"]["tb_per_s_of_w"] = round(4 * n * k / res[f"r{r}"]["median_ms"] / 1e9, 3)
            per_expert[r] += res[f"r{r}"]["median_ms"] * (8 if name == "D->D" else 1) * 40
        out[name] = res
        del w, variants
        torch.cuda.empty_cache()
    out["per_expert_ms_extrapolated_from_repeated_calls"] = {f"r{r}": round(v, 2) for r, v in per_expert.items()}
    out["per_expert_gb_of_w"] = round(40 * 4 * (8 * DIM * DIM + 2 * DIM * FFN) / 1e9, 2)
    return out


def expert_leg(torch, ops, passes, ranks, layers=40):
    """One pass of gf_lora_merge over the 10 x `layers` DISTINCT weights of an expert's blocks (28 GB at 40 layers: every weight comes
    from HBM, none from the Infinity Cache), between two events; `passes` passes per rank, the factors shared per shape."""
    g = torch.Generator(device="cuda").manual_seed(5)
    shapes = [(DIM, DIM)] * 8 + [(FFN, DIM), (DIM, FFN)]
    ws = [torch.empty(s, device="cuda", dtype=torch.bfloat16).normal_(0, s[1] ** -0.5, generator=g) for _ in range(layers) for s in shapes]
    moved = sum(4 * w.numel() for w in ws)
    out = {"weights": len(ws), "gb_moved": round(moved / 1e9, 2)}
    for r in ranks:
        fac = {s: ((torch.randn((s[0], r), device="cuda", generator=g) / s[1] ** 0.5).to(torch.bfloat16),
                   (torch.randn((r, s[1]), device="cuda", generator=g) / r ** 0.5).to(torch.bfloat16)) for s in set(shapes)}

        def one_pass():
            for w in ws:
                ops.lora_merge(w, *fac[tuple(w.shape)], 1e-3)
        res = summary([timed(torch, one_pass, 1) for _ in range(passes + 1)][1:])
        res["tb_per_s_of_w"] = round(moved / res["median_ms"] / 1e9, 3)
        out[f"r{r}"] = res
    return out


def step_leg(torch, rounds, layers, rank):
    from goal_force_amd import dit as D
    from goal_force_amd import lora
    from goal_force_amd.pipeline import WanVideoPipeline, build_random_controlnet, build_random_expert
    dev = torch.device("cuda", 0)
    cfg = dict(D.A14B_CONFIG)
    cfg["num_layers"] = layers
    n_cn = min(10, layers)
    mods = (build_random_expert(cfg, seed=100, device=dev), build_random_expert(cfg, seed=200, device=dev),
            build_random_controlnet(n_cn, cfg, seed=300, device=dev), build_random_controlnet(n_cn, cfg, seed=400, device=dev, zero_convs_zero=True))
    pipe = WanVideoPipeline.from_modules(*mods, device=dev)
    g = torch.Generator().manual_seed(1000)
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
    # the high-noise step runs dit and controlnet: adapters for every block of both
    sds = {}
    ag = torch.Generator().manual_seed(24)
    for key, m in (("dit", mods[0]), ("cn", mods[2])):
        sd = {}
        for name, mod in m.named_modules():
            if isinstance(mod, D.DiTBlock):
                for lname in BLOCK_LAYERS:
                    lin = mod.get_submodule(lname)
                    sd.update(adapter_sd(torch, f"{name}.{lname}", lin.weight.shape[0], lin.weight.shape[1], rank, ag))
        sds[key] = sd

    def run():
        pipe.denoise(latents, ctx_p, ctx_n, y, control, num_inference_steps=50, cfg_scale=5.0, controlnet=True, step_ids=[0], record_step_times=True)
        return pipe.last_step_ms[0][0]

    n_att = lora.attach(mods[0], sds["dit"], alpha=0.0) + lora.attach(mods[2], sds["cn"], alpha=0.0)
    modes = {"plain": 0.0, "attached": 0.7, "plain again": 0.0}
    times = {m: [] for m in modes}
    for s in modes.values():
        lora.set_strength(pipe, s)
        run()
    for _ in range(rounds):
        for m, s in modes.items():
            lora.set_strength(pipe, s)
            times[m].append(run())
    res = {m: summary(t) for m, t in times.items()}
    lora.detach(pipe)
    with contextlib.redirect_stdout(sys.stderr):          # (the loader's own line is not part of this tool's JSON)
        n_merged = pipe.load_lora(mods[0], sds["dit"], alpha=0.7) + pipe.load_lora(mods[2], sds["cn"], alpha=0.7)
    run()
    res["merged"] = summary([run() for _ in range(rounds)])
    aa = abs(res["plain"]["median_ms"] - res["plain again"]["median_ms"]) / res["plain"]["median_ms"]
    res["aa_plain_rel"] = round(aa, 4)
    res["noise_rel"] = round(max([aa] + [res[m]["spread"] for m in modes]), 4)
    res["attached_over_plain"] = round(res["attached"]["median_ms"] / res["plain"]["median_ms"], 4)
    res["merged_over_plain"] = round(res["merged"]["median_ms"] / res["plain"]["median_ms"], 4)
    res.update(rank=rank, attached_layers=n_att, merged_layers=n_merged, layers=layers)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--no-steps", action="store_true", help="without the step leg")
    ap.add_argument("--no-layers", action="store_true", help="without the layer and merge legs")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("lora_bench.py measures on the GPU: no HIP device found (there is no fallback)")
    from goal_force_amd import ops
    torch.set_grad_enabled(False)
    if not args.no_layers:
        print(json.dumps({"leg": "layer", "M": S_TOKENS, "rounds": args.rounds, "calls": args.calls,
                          "shapes": layer_leg(torch, ops, args.rounds, args.calls, (16, 64, 128))}), flush=True)
        print(json.dumps({"leg": "merge", "rounds": args.rounds, "calls": args.calls,
                          "shapes": merge_leg(torch, ops, args.rounds, args.calls, (16, 64, 128, 256))}), flush=True)
        torch.cuda.empty_cache()
        print(json.dumps({"leg": "expert_merge", "passes": 3, **expert_leg(torch, ops, 3, (16, 64, 128, 256), args.layers)}), flush=True)
    torch.cuda.empty_cache()
    if not args.no_steps:
        print(json.dumps({"leg": "step", "rounds": args.step_rounds, **step_leg(torch, args.step_rounds, args.layers, 64)}), flush=True)


if __name__ == "__main__":
    main()
