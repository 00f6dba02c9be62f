#!/usr/bin/env python3
"""LoRA training on the device: ops.lora_grad against the route the tree had before it, and an adapted block's backward.

One process, the two routes ALTERNATING call by call, device events around each call, at the training sequence (M = 32760 tokens):

  * `grad`: ops.lora_grad(y, t, s) against training.linear_dw — two transposed, padded copies and the forward GEMM with K = M — for the
    three layer shapes of the A14B expert (D->D, D->F, F->D; D = 5120, F = 13824) at ranks 32 / 64 / 256, both orientations:
        dUp   [n_out, r] : lora_grad(dy [M, n_out], t [M, r])               vs linear_dw(dy, t)
        dDown [r, k_in]  : lora_grad(x [M, k_in], dt [M, r], transposed)    vs linear_dw(dt, x)
    Reported: the median time of each, their ratio, and the new kernel's bytes/s against ONE read of the wide operand (M C 2 bytes:
    the least traffic the product needs; the narrow operand, the partials and the result are not counted), as a share of the
    8 TB/s HBM peak.  The results are compared before anything is timed (the same products: they differ by their roundings only).
  * `block`: forward + backward of ONE A14B-sized block through training.block_forward, frozen (activations only) against the
    same block with all ten Linears adapted at rank 32 (`--block-rank`), 512 context rows.

The yardstick is the parent's route, never an earlier run of the new kernel.  Prints one JSON line per measurement.

    python tools/lora_train_bench.py [--tokens 32760] [--iters 20] [--what grad,block]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, F, HEADS, CTX = 5120, 13824, 40, 512
HBM_PEAK = 8.0e12
SHAPES = (("D->D", D, D), ("D->F", D, F), ("F->D", F, D))         # (name, k_in, n_out)
RANKS = (32, 64, 256)


def _time(fns, iters, torch):
    """Median milliseconds per call of each fn, the calls alternating."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(iters):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[i].append(a.elapsed_time(b))
    return [statistics.median(t) for t in times], [(min(t), max(t)) for t in times]


def bench_grad(args, torch, ops, training):
    M = args.tokens
    g = torch.Generator(device="cuda").manual_seed(1)
    wide = {C: torch.randn((M, C), generator=g, device="cuda", dtype=torch.float32).to(torch.bfloat16) for C in (D, F)}
    for name, k_in, n_out in SHAPES:
        for r in RANKS:
            narrow = (torch.randn((M, r), generator=g, device="cuda") / M ** 0.5).to(torch.bfloat16)
            for kind, C in (("dUp", n_out), ("dDown", k_in)):
                y = wide[C]
                tr = kind == "dDown"
                new = lambda: ops.lora_grad(y, narrow, 1.0, transposed=tr)                                    # noqa: E731
                old = (lambda: training.linear_dw(narrow, y)) if tr else (lambda: training.linear_dw(y, narrow))    # noqa: E731
                a, b = new().float(), old().float()
                rel = float((a - b).norm() / b.norm())
                assert a.shape == b.shape and rel < 1e-2, (name, r, kind, a.shape, b.shape, rel)
                (t_new, t_old), spread = _time([new, old], args.iters, torch)
                bps = M * C * 2 / (t_new * 1e-3)
                print(json.dumps(dict(what="grad", layer=name, rank=r, kind=kind, M=M, C=C, lora_grad_ms=round(t_new, 4),
                                      linear_dw_ms=round(t_old, 4), speedup=round(t_old / t_new, 3), rel_l2_between_routes=rel,
                                      lora_grad_min_max_ms=[round(v, 4) for v in spread[0]], linear_dw_min_max_ms=[round(v, 4) for v in spread[1]],
                                      bytes_per_s_one_read_of_y=round(bps / 1e12, 3), unit="TB/s", share_of_hbm_peak=round(bps / HBM_PEAK, 3))),
                      flush=True)


def bench_block(args, torch, ops, training):
    from goal_force_amd import lora
    from goal_force_amd.dit import DiTBlock, RopeTable, precompute_freqs_cis_3d
    M = args.tokens
    grid = (21, 30, 52) if M == 32760 else (1, 1, M)
    with torch.device("cuda"):
        blk = DiTBlock(False, D, HEADS, F, 1e-6)
    blk = blk.to(torch.bfloat16)
    for p in blk.parameters():
        p.requires_grad_(False)
    rope = RopeTable.from_grid(precompute_freqs_cis_3d(D // HEADS), *grid, "cuda")
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn((M, D), generator=g, device="cuda").to(torch.bfloat16).requires_grad_(True)
    ctx = torch.randn((CTX, D), generator=g, device="cuda").to(torch.bfloat16)
    t_mod = (0.1 * torch.randn((1, 6, D), generator=g, device="cuda")).to(torch.bfloat16)
    dout = torch.randn((M, D), generator=g, device="cuda").to(torch.bfloat16)

    def step():
        x.grad = None
        with torch.enable_grad():
            training.block_forward(blk, x, ctx, t_mod, rope).backward(dout)

    (t_frozen,), (s_frozen,) = _time([step], args.iters // 2 or 1, torch)
    lora.add_trainable(blk, "q,k,v,o,ffn.0,ffn.2", args.block_rank)
    with torch.no_grad():
        for _, _, ad in lora.trainable(blk):
            ad.up[:, :ad.rank] = (0.02 * torch.randn((ad.up.shape[0], ad.rank), device="cuda")).to(torch.bfloat16)
    (t_lora,), (s_lora,) = _time([step], args.iters // 2 or 1, torch)
    print(json.dumps(dict(what="block", M=M, rank=args.block_rank, frozen_fwd_bwd_ms=round(t_frozen, 3), adapted_fwd_bwd_ms=round(t_lora, 3),
                          ratio=round(t_lora / t_frozen, 3), frozen_min_max_ms=[round(v, 3) for v in s_frozen],
                          adapted_min_max_ms=[round(v, 3) for v in s_lora], keep_level="auto")), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=32760)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--block-rank", type=int, default=32)
    ap.add_argument("--what", default="grad,block")
    args = ap.parse_args(argv)
    import torch
    from goal_force_amd import ops, training
    assert torch.cuda.is_available(), "this benchmark measures the device: no GPU, no number"
    torch.set_grad_enabled(False)
    for what in args.what.split(","):
        {"grad": bench_grad, "block": bench_block}[what](args, torch, ops, training)


if __name__ == "__main__":
    main()
