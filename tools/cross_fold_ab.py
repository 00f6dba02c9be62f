#!/usr/bin/env python3
"""Crossover of the cross-attention's two projection paths at the bench shape (S = 32760, D = 5120, 40 heads), both in one process:
  unfolded: flash_attn (kernel 2, last key x m) -> a [S, D];  gemm(a, W_o, b, EPI_BIAS_RESID)                     K = D
  folded  : cross_probs -> P [S, 40 n_pad];                    gemm(P, U, b, EPI_BIAS_RESID), U = cross_fold_table  K = 40 n_pad
for n_keys from 1 to 63 (the range gf_cross_probs takes; n_pad = n_keys + 1 rounded up to 16).  Each launch is bracketed by events;
the two paths alternate, median of --reps.  Prints one line per n_keys and a JSON summary (dit.CrossAttention.FOLD_K_MAX is set from it).

    python tools/cross_fold_ab.py [--reps 20] [--keys 1,17,41,63]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--keys", default="1,15,16,31,32,41,47,48,63")
    ap.add_argument("--tokens", type=int, default=32760)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    S, D, H = args.tokens, 5120, 40
    g = torch.Generator(device="cuda").manual_seed(0)
    bf = torch.bfloat16
    q = torch.randn(S, D, generator=g, device="cuda").to(bf)
    w = (torch.randn(D, D, generator=g, device="cuda") / D ** 0.5).to(bf)
    b = (torch.randn(D, generator=g, device="cuda") * 0.02).to(bf)
    x = torch.randn(S, D, generator=g, device="cuda").to(bf)
    rows = []
    for n in [int(t) for t in args.keys.split(",")]:
        k = torch.randn(n, D, generator=g, device="cuda").to(bf)
        v = torch.randn(n, D, generator=g, device="cuda").to(bf)
        m = 512 - n + 1 if n > 1 else 1
        n_pad = -(-(n + 1) // 16) * 16
        u = ops.cross_fold_table(v, w, H, n_pad)
        a = torch.empty(S, D, dtype=bf, device="cuda")
        p = torch.empty(S, H * n_pad, dtype=bf, device="cuda")
        t = {"attn": [], "gemm_dd": [], "probs": [], "gemm_fold": []}

        def timed(name, fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            t[name].append((e0, e1))

        for _ in range(args.reps + 2):
            timed("attn", lambda: ops.flash_attn(q, k, v, H, out=a, last_key_mult=m))
            timed("gemm_dd", lambda: ops.gemm(a, w, b, epilogue=ops.EPI_BIAS_RESID, resid=x, out=x))
            timed("probs", lambda: ops.cross_probs(q, k, H, n_pad, last_key_mult=m, out=p))
            timed("gemm_fold", lambda: ops.gemm(p, u, b, epilogue=ops.EPI_BIAS_RESID, resid=x, out=x))
        torch.cuda.synchronize()
        med = {key: statistics.median(e0.elapsed_time(e1) for e0, e1 in ev[2:]) for key, ev in t.items()}
        old, new = med["attn"] + med["gemm_dd"], med["probs"] + med["gemm_fold"]
        kf = H * n_pad
        r = dict(n_keys=n, n_pad=n_pad, K_fold=kf, attn_ms=med["attn"], gemm_dd_ms=med["gemm_dd"], probs_ms=med["probs"],
                 gemm_fold_ms=med["gemm_fold"], unfolded_ms=old, folded_ms=new, speedup=old / new,
                 gemm_fold_tflops=2.0 * S * D * kf / med["gemm_fold"] / 1e9, gemm_dd_tflops=2.0 * S * D * D / med["gemm_dd"] / 1e9)
        rows.append(r)
        print(f"n_keys {n:3d} (K {kf:4d}): unfolded {old:.3f} ms (attn {med['attn']:.3f} + gemm {med['gemm_dd']:.3f}) | folded {new:.3f} ms "
              f"(probs {med['probs']:.3f} + gemm {med['gemm_fold']:.3f}, {r['gemm_fold_tflops']:.0f} TFLOP/s) | x{old / new:.2f}", flush=True)
    print(json.dumps({"tool": "cross_fold_ab", "tokens": S, "dim": D, "heads": H, "reps": args.reps, "rows": rows}))


if __name__ == "__main__":
    main()
