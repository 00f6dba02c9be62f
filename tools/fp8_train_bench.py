#!/usr/bin/env python3
"""Training through frozen fp8 blocks against the bf16 tape, in ONE process with the arms alternating (a measurement tool, not the
driver's bench contract; profiles/r27).  At the A14B widths and M = 32760 tokens:

  dx      training.linear_dx (bf16: transpose + GEMM) against training.linear_dx_fp8 per layer shape, with ops.quant_fp8_grad alone;
  block   one frozen block's forward + backward, bf16 against fp8-frozen, at each keep level; the extra bytes of the fp8 copies;
          rel-L2 and cosine of dx between the two arms (a number, not a quality claim);
  step    the ControlNet step of tools/train_bench.py under both arms (--layers / --cn-layers as there).

  python3 tools/fp8_train_bench.py dx block
  python3 tools/fp8_train_bench.py step --layers 4 --cn-layers 2

Every figure is the median of --reps alternating repetitions after one untimed pass per arm; one JSON line per section."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from goal_force_amd import dit, ops, training as tr  # noqa: E402
from goal_force_amd.dit import A14B_CONFIG  # noqa: E402

S, D, F, L = 32760, 5120, 13824, 512
BF = torch.bfloat16
LAYERS = {"q/k/v/o": (D, D), "ffn.0": (F, D), "ffn.2": (D, F)}          # name -> (out_features, in_features)


def timed(arms, reps):
    """{name: median ms} of the callables in `arms`, run alternately: one untimed pass each, then `reps` rounds."""
    for f in arms.values():
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, f in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: statistics.median(v) for k, v in ms.items()}


def switch(module, fp8):
    """Put `module`'s blocks in an arm, outside the timed region: the e4m3 copies and (made once per weight, on the first backward, in
    real use) their transposed copies, or none; and the tape's switch."""
    dit.enable_fp8(module, fp8)
    tr.set_fp8_frozen(fp8)
    if fp8:
        for blk in (m for m in module.modules() if isinstance(m, dit.DiTBlock)):
            for lin in (m for m in blk.modules() if isinstance(m, torch.nn.Linear)):
                dit.fp8_weight_t(lin)


def bench_dx(a, dev):
    g = torch.Generator().manual_seed(1)
    out = {}
    for name, (n, k) in LAYERS.items():
        lin = torch.nn.Linear(k, n, bias=False).to(BF).to(dev)
        lin.weight.requires_grad_(False)
        dit.weight_copy(lin, "fp8", True)
        dy = (torch.randn((a.tokens, n), generator=g) * 2.0 ** -10).to(BF).to(dev)
        dit.fp8_weight_t(lin)                                   # made once per weight, outside the timed region
        t = timed({"bf16": lambda: tr.linear_dx(dy, lin.weight), "fp8": lambda: tr.linear_dx_fp8(dy, lin),
                   "quant": lambda: ops.quant_fp8_grad(dy)}, a.reps)
        out[name] = {"N": n, "K": k, **{f"{kk}_ms": round(v, 4) for kk, v in t.items()}, "speedup": round(t["bf16"] / t["fp8"], 3),
                     "quant_share": round(t["quant"] / t["fp8"], 3)}
        del lin, dy
    print(json.dumps({"section": "dx", "tokens": a.tokens, "layers": out}))


def bench_block(a, dev):
    torch.manual_seed(2)
    blk = dit.DiTBlock(False, D, A14B_CONFIG["num_heads"], F, 1e-6).to(BF).to(dev)
    for p in blk.parameters():
        p.requires_grad_(False)
    f_, h_, w_ = a.tokens // (30 * 52), 30, 52
    rope = dit.RopeTable.from_grid(dit.precompute_freqs_cis_3d(D // A14B_CONFIG["num_heads"]), f_, h_, w_, dev)
    tokens = f_ * h_ * w_
    g = torch.Generator().manual_seed(3)
    x = torch.randn((tokens, D), generator=g).to(BF).to(dev)
    ctx = torch.randn((L, D), generator=g).to(BF).to(dev)
    t_mod = (0.1 * torch.randn((1, 6, D), generator=g)).to(BF).to(dev)
    dout = (torch.randn((tokens, D), generator=g) * 2.0 ** -10).to(BF).to(dev)
    dx = {}

    def arm(fp8):
        def run():
            switch(blk, fp8)
            xg = x.clone().requires_grad_(True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            with torch.enable_grad():
                tr.block_forward(blk, xg, ctx, t_mod, rope).backward(dout)
            e1.record()
            e1.synchronize()
            dx[fp8] = xg.grad
            return e0.elapsed_time(e1)
        return run

    base = torch.cuda.memory_allocated()
    switch(blk, True)
    extra = torch.cuda.memory_allocated() - base
    params = sum(m.weight.numel() for m in blk.modules() if isinstance(m, torch.nn.Linear))
    out = {"section": "block", "tokens": tokens, "linear_params": params, "fp8_copies_bytes": extra, "levels": {}}
    for level in ("none", "attn", "wide"):
        old = tr.set_keep_level(level)
        arms = {"bf16": arm(False), "fp8": arm(True)}
        for f in arms.values():
            f()
        ms = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, f in arms.items():
                ms[k].append(f())
        tr.set_keep_level(old)
        med = {k: statistics.median(v) for k, v in ms.items()}
        d = (dx[True].double() - dx[False].double())
        out["levels"][level] = {"bf16_ms": round(med["bf16"], 3), "fp8_ms": round(med["fp8"], 3), "speedup": round(med["bf16"] / med["fp8"], 3),
                                "dx_rel_l2": float(d.norm() / dx[False].double().norm()),
                                "dx_cosine": float(torch.nn.functional.cosine_similarity(dx[True].double().flatten(), dx[False].double().flatten(), dim=0))}
    tr.set_fp8_frozen(False)
    print(json.dumps(out))


def bench_step(a, dev):
    from goal_force_amd.pipeline import WanVideoPipeline, build_random_controlnet, build_random_expert
    cfg = dict(A14B_CONFIG)
    cfg["num_layers"] = a.layers
    expert = build_random_expert(cfg, seed=100, device=dev)
    for p in expert.parameters():
        p.requires_grad_(False)
    cn = build_random_controlnet(a.cn_layers, cfg, seed=300, device=dev)
    pipe = WanVideoPipeline.from_modules(expert, None, cn, None, device=dev)
    pipe.scheduler.set_timesteps(1000, training=True)
    g = torch.Generator().manual_seed(0)
    shp = (1, 16, a.tokens // (30 * 52), 60, 104)
    inp = dict(input_latents=torch.randn(shp, generator=g), noise=torch.randn(shp, generator=g), y=torch.randn((1, 20) + shp[2:], generator=g),
               control=torch.randn(shp, generator=g), context=torch.randn((1, L, 4096), generator=g))
    inp = {k: v.to(BF).to(dev) for k, v in inp.items()}

    def arm(fp8):
        def run():
            switch(expert, fp8)
            for p in cn.parameters():
                p.grad = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            with torch.enable_grad():
                loss = tr.training_loss(pipe, input_latents=inp["input_latents"], noise=inp["noise"], context=inp["context"], y=inp["y"],
                                        control_signal_video_latents=inp["control"], timestep_id=500)
            loss.backward()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1), float(loss.detach())
        return run

    arms = {"bf16": arm(False), "fp8": arm(True)}
    for f in arms.values():
        f()
    ms, loss = {k: [] for k in arms}, {}
    for _ in range(a.reps):
        for k, f in arms.items():
            t, loss[k] = f()
            ms[k].append(t)
    tr.set_fp8_frozen(False)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"section": "step", "layers": a.layers, "controlnet_layers": a.cn_layers, "tokens": a.tokens,
                      "bf16_fwd_bwd_s": round(med["bf16"] / 1e3, 4), "fp8_fwd_bwd_s": round(med["fp8"] / 1e3, 4),
                      "speedup": round(med["bf16"] / med["fp8"], 3), "loss_bf16": loss["bf16"], "loss_fp8": loss["fp8"],
                      "peak_mem_gb": torch.cuda.max_memory_allocated() / 2 ** 30}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sections", nargs="+", choices=("dx", "block", "step"))
    ap.add_argument("--tokens", type=int, default=S)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--cn-layers", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for s in a.sections:
        {"dx": bench_dx, "block": bench_block, "step": bench_step}[s](a, dev)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
