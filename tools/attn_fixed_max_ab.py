#!/usr/bin/env python3
"""A/B of kernel 3's two softmax schedules in ONE process and ONE library: the running maximum in one launch
(options(attn_fixed_max=0), the parent's path) against the fixed-maximum launch + repair launch (the default), alternating
launch by launch on the same operands.
    python3 tools/attn_fixed_max_ab.py [--s 32760] [--pairs 16] [--qscale 8] [--ramp 8] [--out FILE]
Prints, per data set, one JSON line: both medians, each arm's min-to-max spread, the blocks repaired and the rel-L2 between the
two outputs.  --early-exit: also an upper bound for a repair launch that finds nothing to do (early_exit())."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from goal_force_amd import ops

D, H = 5120, 40
BF = torch.bfloat16


def pair_times(q, k, v, pairs):
    """Alternating launches: exact, fixed, exact, fixed, ...; returns ({arm: [ms]}, outputs, repaired blocks)."""
    o = {a: torch.empty_like(q) for a in ("exact", "fixed")}
    flags = None
    for a in ("exact", "fixed"):          # warm-up: both code objects loaded, V^T workspace allocated
        with ops.options(attn_fixed_max=int(a == "fixed")):
            ops.flash_attn(q, k, v, H, out=o[a])
            if a == "fixed":
                flags = ops.last_attn_flags
    torch.cuda.synchronize()
    evs = {"exact": [], "fixed": []}
    for _ in range(pairs):
        for a in ("exact", "fixed"):
            with ops.options(attn_fixed_max=int(a == "fixed")):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.flash_attn(q, k, v, H, out=o[a])
                e1.record()
                evs[a].append((e0, e1))
    torch.cuda.synchronize()
    ts = {a: [e0.elapsed_time(e1) for e0, e1 in evs[a]] for a in evs}
    repaired = int((flags != 0).any(dim=2).sum())
    return ts, o, repaired, flags.shape[0] * flags.shape[1]


def report(name, ts, o, repaired, blocks):
    med = {a: sorted(t)[len(t) // 2] for a, t in ts.items()}
    row = {"data": name, "pairs": len(ts["exact"]), "blocks": blocks, "blocks_repaired": repaired,
           "rel_l2_fixed_vs_exact": float((o["fixed"].float() - o["exact"].float()).norm() / o["exact"].float().norm()),
           "finite": bool(torch.isfinite(o["fixed"].float()).all())}
    for a, t in ts.items():
        row[a] = {"median_ms": round(med[a], 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                  "spread_ms": round(max(t) - min(t), 4)}
    row["gain_ms"] = round(med["exact"] - med["fixed"], 4)
    row["gain_pct"] = round(100.0 * (med["exact"] - med["fixed"]) / med["exact"], 3)
    row["gain_above_exact_spread"] = bool(row["gain_ms"] > row["exact"]["spread_ms"])
    print(json.dumps(row), flush=True)
    return row


def early_exit(s, iters):
    """What a repair launch costs when every workgroup finds eight zero flags and returns: the _fm pair against the plain entry
    point at 128 keys (two tiles, the shortest the kernel takes) on the production query grid — the first launches do the same
    two tiles of work, the difference is the second launch (an upper bound: it includes what the two first kernels differ by)."""
    from goal_force_amd import _lib
    lib = _lib.load()
    skv, kvp = 128, 128
    q = torch.randn((s, D), device="cuda").to(BF)
    k = torch.randn((skv, D), device="cuda").to(BF)
    v = torch.randn((skv, D), device="cuda").to(BF)
    vt = torch.empty((H * 128 * kvp,), dtype=BF, device="cuda")
    o = torch.empty_like(q)
    flags = torch.empty((H * (-(-s // 256)) * 8,), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.gf_transpose_v32(v.data_ptr(), D, vt.data_ptr(), skv, kvp, H, st), "gf_transpose_v32")
    tail = (s, skv, kvp, H, 128, D, D, D, 128 ** -0.5, st)

    def exact():
        _lib.check(lib.gf_flash_attn_fwd_vt32(q.data_ptr(), k.data_ptr(), vt.data_ptr(), o.data_ptr(), None, *tail), "vt32")

    def fm():
        _lib.check(lib.gf_flash_attn_fwd_vt32_fm(q.data_ptr(), k.data_ptr(), vt.data_ptr(), o.data_ptr(), None, flags.data_ptr(), *tail), "vt32_fm")
    ts = {"exact": [], "fm": []}
    for fn in (exact, fm):
        fn()
    torch.cuda.synchronize()
    evs = {"exact": [], "fm": []}
    for _ in range(iters):
        for name, fn in (("exact", exact), ("fm", fm)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs[name].append((e0, e1))
    torch.cuda.synchronize()
    ts = {a: sorted(e0.elapsed_time(e1) for e0, e1 in evs[a]) for a in evs}
    row = {"data": "early-exit repair launch (128 keys, production query grid)", "exact_one_launch_median_ms": round(ts["exact"][iters // 2], 4),
           "fm_two_launches_median_ms": round(ts["fm"][iters // 2], 4),
           "repair_exit_upper_bound_ms": round(ts["fm"][iters // 2] - ts["exact"][iters // 2], 4), "flags_set": int((flags != 0).sum())}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=32760)
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--qscale", type=float, default=0.0, help="also: logits x f (8 = bench.py's peaky leg)")
    ap.add_argument("--ramp", type=float, default=0.0, help="also: tools/microbench.py's adversarial ramp (every block overflows and is repaired)")
    ap.add_argument("--early-exit", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    s = a.s
    q = torch.randn((s, D), device="cuda").to(BF)
    k = torch.randn((s, D), device="cuda").to(BF)
    v = torch.randn((s, D), device="cuda").to(BF)
    rows = [report("random (logit std 1)", *pair_times(q, k, v, a.pairs))]
    if a.qscale > 0:
        q8 = (q.float() * a.qscale).to(BF)
        rows.append(report(f"logits x {a.qscale:g}", *pair_times(q8, k, v, a.pairs)))
    if a.ramp > 0:
        hd = D // H
        tiles = (s + 63) // 64
        amp = math.sqrt(a.ramp * tiles * math.log(2.0) * math.sqrt(hd))
        u = torch.ones((hd,), device="cuda") / math.sqrt(hd)
        qr = (amp * u).repeat(H)[None, :].expand(s, D).contiguous().to(BF)
        kr = ((torch.arange(s, device="cuda", dtype=torch.float32) / s)[:, None] * (amp * u).repeat(H)[None, :]).to(BF)
        rows.append(report(f"ramp +{a.ramp:g} log2 units per tile", *pair_times(qr, kr, v, max(4, a.pairs // 2))))
    rows.append(report("random again", *pair_times(q, k, v, a.pairs)))
    if a.early_exit:
        rows.append(early_exit(s, 20))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
