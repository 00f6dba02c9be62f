"""One-process A/B of the SageAttention backend against attention kernel 3 (profiles/r08).

(a) the self-attention at the production shape (S = 32760, 40 heads, random bf16 operands, q pre-scaled as the blocks produce it):
    kernel 3 with V^T from the projection (gf_flash_attn_fwd_vt32) against the four sage quantisation passes and gf_sage_attn_fwd,
    each timed separately, and the whole ops.sage_attn; --pairs interleaved rounds, the median of --iters launches per leg.
(b) --step: one high-noise denoise step (cond + uncond, 40 DiT + 10 ControlNet blocks at 32760 tokens, random weights built by
    tests/fullsize_parity.py) with enable_sage_attention off and on, in bf16 and with fp8 linears; --pairs interleaved pairs.
One JSON line per part.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from goal_force_amd import ops  # noqa: E402

BF = torch.bfloat16


def timeit(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    fn()
    torch.cuda.synchronize()
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return t[len(t) // 2]


def kernel_ab(pairs, iters):
    s, h = 32760, 40
    d = h * 128
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn((s, d), generator=g, device="cuda").to(BF)
    c = float(torch.tensor(1.0 / math.sqrt(128)) * torch.tensor(1.4426950408889634))
    q = (torch.randn((s, d), generator=g, device="cuda") * c).to(BF)
    k = torch.randn((s, d), generator=g, device="cuda").to(BF)
    w = (torch.randn((d, d), generator=g, device="cuda") / math.sqrt(d)).to(BF)
    vt = ops.linear_vt32(x, w, None).clone()
    o = torch.empty((s, d), dtype=BF, device="cuda")
    ln2 = math.log(2.0)
    flops = 4.0 * s * s * 128 * h
    mu = ops.sage_k_mean(k, h)
    q8, qs = ops.sage_quant_q(q, h)
    k8, ks, _ = ops.sage_quant_k(k, h, mu)
    vt8, vs = ops.sage_quant_vt(None, h, vt=vt, kv_len=s)
    legs = {
        "k3": lambda: ops.flash_attn(q, k, None, h, vt=vt, scale=ln2, out=o),
        "sage_total": lambda: ops.sage_attn(q, k, None, h, vt=vt, scale=ln2, out=o),
        "sage_attn_fwd": lambda: ops.sage_attn_quantized(q8, qs, k8, ks, vt8, vs, s, h, scale=ln2, out=o),
        "k_mean": lambda: ops.sage_k_mean(k, h),
        "quant_q": lambda: ops.sage_quant_q(q, h),
        "quant_k": lambda: ops.sage_quant_k(k, h, mu),
        "quant_vt": lambda: ops.sage_quant_vt(None, h, vt=vt, kv_len=s),
    }
    res = {n: [] for n in legs}
    for _ in range(pairs):
        for n, f in legs.items():
            res[n].append(timeit(f, iters))
    out = {"shape": {"S": s, "heads": h}, "device": torch.cuda.get_device_name(0), "ms": res}
    for n in ("k3", "sage_total", "sage_attn_fwd"):
        best = min(res[n])
        out[f"{n}_tflops_best"] = flops / best / 1e9
    out["sage_attn_fwd_frac_of_int8_fp8_peak"] = out["sage_attn_fwd_tflops_best"] / 5000.0
    out["k3_frac_of_bf16_peak"] = out["k3_tflops_best"] / 2500.0
    out["speedup_total_vs_k3_per_pair"] = [a / b for a, b in zip(res["k3"], res["sage_total"])]
    print(json.dumps(out))


def step_ab(pairs):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import fullsize_parity as fp
    from goal_force_amd.dit import enable_fp8, enable_sage_attention
    dev = torch.device("cuda", torch.cuda.current_device())
    _, pipe = fp.build(40, 10, dev, need_low=False)
    inp = fp.inputs(pipe, (21, 60, 104), dev)

    def step():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pipe.denoise(inp["latents"], inp["ctx_p"], inp["ctx_n"], inp["y"], inp["control"], num_inference_steps=50, cfg_scale=5.0,
                     controlnet=True, step_ids=[12])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    res = {}
    for f8 in (False, True):
        for m in (pipe.dit, pipe.controlnet):
            enable_fp8(m, f8)
        for sage in (False, True):                  # warm-up of both paths (workspaces, weight casts, context cache)
            for m in (pipe.dit, pipe.controlnet):
                enable_sage_attention(m, sage)
            step()
        for _ in range(pairs):
            for sage in (False, True):
                for m in (pipe.dit, pipe.controlnet):
                    enable_sage_attention(m, sage)
                res.setdefault(f"{'fp8' if f8 else 'bf16'}_{'sage' if sage else 'k3'}", []).append(step())
    out = {"step_ms": res, "device": torch.cuda.get_device_name(0),
           "what": "one high-noise step (step id 12 of 50): cond + uncond model_fn, 40 + 10 blocks, 32760 tokens, CFG + Euler"}
    for f8 in ("bf16", "fp8"):
        out[f"{f8}_speedup_per_pair"] = [a / b for a, b in zip(res[f"{f8}_k3"], res[f"{f8}_sage"])]
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step", action="store_true", help="part (b) only: the full denoise step")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    if a.step:
        step_ab(a.pairs)
    else:
        kernel_ab(a.pairs, a.iters)
