#!/usr/bin/env python3
"""MXFP4 linears against the fp8 and bf16 GEMMs of the same library, in ONE process, alternating (profiles/r15/README.md,
profiles/r16/README.md).

  GEMM leg   M = 32760 at (N, K) = (13824, 5120), (5120, 13824), (5120, 5120): gf_gemm_mxfp4, its two quantiser passes' activation share
             (gf_quant_mxfp4 on [M, K]; the weight copy is made once, at enable_fp4) and, for the same accounting, gf_quant_fp8_rowscale,
             against gf_gemm_fp8 and gf_gemm_bf16; gf_gemm_fp8 twice (A/A) for the run-to-run spread.  Every variant is warmed, then
             timed in `--rounds` alternating rounds of `--calls` calls between two events; median, minimum and (max - min) / median.
  producer   M = 32760: the two fused producers of the FFN's fp4 operands against the pairs they replace —
  leg        layernorm_modulate(scale + shift) + quant_mxfp4 on [M, 5120] against layernorm_modulate_mxfp4, and gemm_mxfp4(GELU) at D->F +
             quant_mxfp4 on [M, 13824] against gemm_mxfp4_q4; each pair timed as a pair, the pair twice (A/A) for the spread; the outputs
             compared bit for bit.
  step leg   one high-noise step of the bench configuration (A14B experts, 10-layer ControlNets, 21 x 60 x 104 latents, CFG) under bf16,
             fp8 (enable_fp8, twice: A/A), fp8 + enable_fp4(("ffn", "o")) with ops.options(fp4_fused=False) and the same fused,
             alternating; then the latents after `--latent-steps` steps of each, their rel-L2 from the bf16 latents and whether the
             fused and unfused latents are equal bit for bit.  Random-init weights: a number, not a quality claim.
Prints one JSON line per leg; needs an MI355X (no fallback).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S_TOKENS, DIM, FFN = 32760, 5120, 13824
SHAPES = {"D->F": (FFN, DIM), "F->D": (DIM, FFN), "D->D": (DIM, DIM)}


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


def gemm_leg(torch, ops, rounds, calls):
    out = {}
    for name, (n, k) in SHAPES.items():
        g = torch.Generator(device="cuda").manual_seed(n + k)
        x = torch.randn((S_TOKENS, k), device="cuda", generator=g).to(torch.bfloat16)
        w = (torch.randn((n, k), device="cuda", generator=g) / k ** 0.5).to(torch.bfloat16)
        y = torch.empty((S_TOKENS, n), device="cuda", dtype=torch.bfloat16)
        x4, xs = ops.quant_mxfp4(x)
        w4, ws = ops.quant_mxfp4(w)
        x8, rs = ops.quant_fp8_rowscale(x)
        w8 = ops.cast_fp8(w)
        variants = {
            "gemm_mxfp4": lambda: ops.gemm_mxfp4(x4, xs, w4, ws, out=y),
            "quant_mxfp4": lambda: ops.quant_mxfp4(x),
            "gemm_fp8": lambda: ops.gemm_fp8(x8, rs, w8, out=y),
            "quant_fp8": lambda: ops.quant_fp8_rowscale(x),
            "gemm_bf16": lambda: ops.gemm(x, w, out=y),
            "gemm_fp8_again": lambda: ops.gemm_fp8(x8, rs, w8, out=y),
        }
        times = {v: [] for v in variants}
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for v, fn in variants.items():
                times[v].append(timed(torch, fn, calls))
        res = {v: summary(t) for v, t in times.items()}
        fl = 2.0 * S_TOKENS * n * k
        for v in ("gemm_mxfp4", "gemm_fp8", "gemm_bf16"):
            res[v]["tflops"] = round(fl / res[v]["median_ms"] / 1e9, 1)
        aa = abs(res["gemm_fp8"]["median_ms"] - res["gemm_fp8_again"]["median_ms"]) / res["gemm_fp8"]["median_ms"]
        noise = max(aa, res["gemm_fp8"]["spread"], res["gemm_fp8_again"]["spread"])
        fp4_total = res["gemm_mxfp4"]["median_ms"] + res["quant_mxfp4"]["median_ms"]
        fp8_total = res["gemm_fp8"]["median_ms"] + res["quant_fp8"]["median_ms"]
        res["aa_fp8_rel"] = round(aa, 4)
        res["noise_rel"] = round(noise, 4)
        res["fp4_with_quant_ms"], res["fp8_with_quant_ms"] = round(fp4_total, 4), round(fp8_total, 4)
        res["fp4_over_fp8_gemm_only"] = round(res["gemm_fp8"]["median_ms"] / res["gemm_mxfp4"]["median_ms"], 3)
        res["fp4_over_fp8_with_quant"] = round(fp8_total / fp4_total, 3)
        res["fp4_faster_than_fp8_beyond_noise"] = bool(fp4_total < fp8_total * (1 - noise))
        res["quant_share_of_fp4_linear"] = round(res["quant_mxfp4"]["median_ms"] / fp4_total, 3)
        out[name] = res
        del x, w, y, x4, xs, w4, ws, x8, rs, w8
        torch.cuda.empty_cache()
    return out


def producer_leg(torch, ops, rounds, calls):
    g = torch.Generator(device="cuda").manual_seed(16)
    x = torch.randn((S_TOKENS, DIM), device="cuda", generator=g).to(torch.bfloat16)
    scale1p = (1 + 0.1 * torch.randn(DIM, device="cuda", generator=g)).to(torch.bfloat16)
    shift = (0.1 * torch.randn(DIM, device="cuda", generator=g)).to(torch.bfloat16)
    w4, ws = ops.quant_mxfp4((torch.randn((FFN, DIM), device="cuda", generator=g) / DIM ** 0.5).to(torch.bfloat16))
    bias = (0.1 * torch.randn(FFN, device="cuda", generator=g)).to(torch.bfloat16)
    h = torch.empty_like(x)
    f = torch.empty((S_TOKENS, FFN), device="cuda", dtype=torch.bfloat16)
    x4, xs = ops.quant_mxfp4(ops.layernorm_modulate(x, scale1p=scale1p, shift=shift, out=h))
    gelu = ops.EPI_BIAS_GELU_TANH

    def ln_pair():
        return ops.quant_mxfp4(ops.layernorm_modulate(x, scale1p=scale1p, shift=shift, out=h))

    def gemm_pair():
        return ops.quant_mxfp4(ops.gemm_mxfp4(x4, xs, w4, ws, bias, epilogue=gelu, out=f))

    variants = {
        "ln_pair": ln_pair, "ln_fused": lambda: ops.layernorm_modulate_mxfp4(x, scale1p=scale1p, shift=shift), "ln_pair_again": ln_pair,
        "gemm_pair": gemm_pair, "gemm_fused": lambda: ops.gemm_mxfp4_q4(x4, xs, w4, ws, bias, epilogue=gelu), "gemm_pair_again": gemm_pair,
    }
    same = {}
    for name in ("ln", "gemm"):
        (a4, a_s), (b4, b_s) = variants[name + "_pair"](), variants[name + "_fused"]()
        same[name] = bool(torch.equal(a4, b4) and torch.equal(a_s, b_s))
    times = {v: [] for v in variants}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for v, fn in variants.items():
            times[v].append(timed(torch, fn, calls))
    res = {v: summary(t) for v, t in times.items()}
    for name in ("ln", "gemm"):
        pair, again, fused = (res[f"{name}_{v}"] for v in ("pair", "pair_again", "fused"))
        aa = abs(pair["median_ms"] - again["median_ms"]) / pair["median_ms"]
        noise = max(aa, pair["spread"], again["spread"])
        res[name] = dict(bits_equal=same[name], aa_rel=round(aa, 4), noise_rel=round(noise, 4),
                         pair_over_fused=round(pair["median_ms"] / fused["median_ms"], 3),
                         saved_ms=round(pair["median_ms"] - fused["median_ms"], 4),
                         fused_not_slower_beyond_noise=bool(fused["median_ms"] <= pair["median_ms"] * (1 + noise)))
    return res


def step_leg(torch, rounds, latent_steps, layers):
    from goal_force_amd import ops
    from goal_force_amd import dit as D
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

    def switch(mode):
        for m in mods:
            D.enable_fp4(m, False)
            D.enable_fp8(m, mode != "bf16")
            if mode.startswith("fp8+fp4"):
                D.enable_fp4(m, True, layers=("ffn", "o"))
        return ops.options(fp4_fused=not mode.endswith("unfused"))

    def run(ids, n_sched=50):
        return pipe.denoise(latents, ctx_p, ctx_n, y, control, num_inference_steps=n_sched, cfg_scale=5.0, controlnet=True, step_ids=ids,
                            record_step_times=True)

    modes = ("bf16", "fp8", "fp8+fp4 unfused", "fp8+fp4 fused", "fp8 again")
    times = {m: [] for m in modes}
    for m in modes:                      # warm every mode
        with switch(m):
            run([0])
    for _ in range(rounds):
        for m in modes:
            with switch(m):
                run([0])
            times[m].append(pipe.last_step_ms[0][0])
    res = {m: summary(t) for m, t in times.items()}
    aa = abs(res["fp8"]["median_ms"] - res["fp8 again"]["median_ms"]) / res["fp8"]["median_ms"]
    noise = max([aa] + [r["spread"] for r in res.values()])
    res["aa_fp8_rel"], res["noise_rel"] = round(aa, 4), round(noise, 4)
    fp8_ms, unfused_ms, fused_ms = (res[m]["median_ms"] for m in ("fp8", "fp8+fp4 unfused", "fp8+fp4 fused"))
    res["fp8_step_over_fused_step"] = round(fp8_ms / fused_ms, 4)
    res["fp8_step_over_unfused_step"] = round(fp8_ms / unfused_ms, 4)
    res["unfused_step_over_fused_step"] = round(unfused_ms / fused_ms, 4)
    res["fused_step_faster_than_fp8_beyond_spread"] = bool(fused_ms < fp8_ms * (1 - noise))
    res["fused_step_faster_than_unfused_beyond_spread"] = bool(fused_ms < unfused_ms * (1 - noise))
    if latent_steps > 0:
        finals = {}
        for m in modes[:-1]:
            with switch(m):
                finals[m] = pipe.denoise(latents, ctx_p, ctx_n, y, control, num_inference_steps=latent_steps, cfg_scale=5.0, controlnet=True)
        ref = finals["bf16"].float()
        res["latents_rel_l2_from_bf16"] = {m: round(float((finals[m].float() - ref).norm() / ref.norm()), 5) for m in modes[1:-1]}
        res["fused_latents_equal_unfused_bit_for_bit"] = bool(torch.equal(finals["fp8+fp4 fused"], finals["fp8+fp4 unfused"]))
        res["latent_steps"] = latent_steps
    switch("bf16")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--latent-steps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--no-steps", action="store_true", help="without the step leg")
    ap.add_argument("--no-gemm", action="store_true", help="without the GEMM leg")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fp4_ab.py measures on the GPU: no HIP device found (there is no fallback)")
    from goal_force_amd import ops
    torch.set_grad_enabled(False)
    if not args.no_gemm:
        print(json.dumps({"leg": "gemm", "M": S_TOKENS, "rounds": args.rounds, "calls": args.calls, "shapes": gemm_leg(torch, ops, args.rounds, args.calls)}), flush=True)
    print(json.dumps({"leg": "producer", "M": S_TOKENS, "rounds": args.rounds, "calls": args.calls, **producer_leg(torch, ops, args.rounds, args.calls)}), flush=True)
    torch.cuda.empty_cache()
    if not args.no_steps:
        print(json.dumps({"leg": "step", "rounds": args.step_rounds, **step_leg(torch, args.step_rounds, args.latent_steps, args.layers)}), flush=True)


if __name__ == "__main__":
    main()
