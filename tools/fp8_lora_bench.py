#!/usr/bin/env python3
"""An fp8 Linear with one attached LoRA adapter: the plain layer, the adapter by two launches (gf_gemm_fp8 + gf_lora_up) and fused
(gf_gemm_fp8_lora), per layer shape and rank — one process, the arms alternating, medians, and the plain arm timed twice for the A/A
spread (as tools/lora_bench.py does).  The rank-wide `t` GEMM is the same in both adapted arms and is timed on its own.

    python tools/fp8_lora_bench.py [--tokens 32760] [--reps 9] [--inner 5] [--parent-lib path/to/the/parent's/libgoalforce_hip.so]

--parent-lib: the plain gf_gemm_fp8 of another build of the library (the parent commit's), loaded beside this one and launched on the
same operands as a further alternating arm: the plain kernel must sit inside the A/A spread of the parent's.

Prints one line per (shape, rank) and the decision rule's verdict: the fused arm must beat the two-launch arm by more than the A/A spread.

    python tools/fp8_lora_bench.py --block          # one A14B-sized block, forward + backward at 32760 tokens: frozen fp8 / frozen fp8 with
                                                    # ten trainable rank-32 adapters beside it / bf16 with the same adapters
    python tools/fp8_lora_bench.py --step           # a high-noise CFG step under enable_fp8, every block Linear attached at rank 64:
                                                    # plain fp8 / attached beside fp8 / plain again, then bf16 attached"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from goal_force_amd import ops  # noqa: E402

BF = torch.bfloat16
D, F = 5120, 13824
SHAPES = (("D->D gate+resid", D, D, ops.EPI_BIAS_GATE_RESID), ("D->F gelu", F, D, ops.EPI_BIAS_GELU_TANH), ("F->D gate+resid", D, F, ops.EPI_BIAS_GATE_RESID),
          ("D->D bias", D, D, ops.EPI_BIAS))
RANKS = (16, 32, 64)


def median(v):
    return sorted(v)[len(v) // 2]


BLOCK_LAYERS = tuple(f"{a}.{p}" for a in ("self_attn", "cross_attn") for p in "qkvo") + ("ffn.0", "ffn.2")


def block_leg(a):
    """Forward + backward of one frozen A14B-sized block (training.block_forward), medians of alternating rounds."""
    from goal_force_amd import dit, lora, training as tr
    dev = "cuda"
    heads = dit.A14B_CONFIG["num_heads"]
    f_, h_, w_ = a.tokens // (30 * 52), 30, 52
    tokens = f_ * h_ * w_
    rope = dit.RopeTable.from_grid(dit.precompute_freqs_cis_3d(D // heads), f_, h_, w_, dev)
    g = torch.Generator().manual_seed(3)
    x = torch.randn((tokens, D), generator=g).to(BF).to(dev)
    ctx = torch.randn((512, D), generator=g).to(BF).to(dev)
    t_mod = (0.1 * torch.randn((1, 6, D), generator=g)).to(BF).to(dev)
    dout = (torch.randn((tokens, D), generator=g) * 2.0 ** -10).to(BF).to(dev)
    old = lora.set_beside_fp8(True), tr.set_fp8_frozen(True), tr.set_keep_level("attn")

    def block(fp8, adapters):
        torch.manual_seed(2)
        blk = dit.DiTBlock(False, D, heads, F, 1e-6).to(BF).to(dev)
        for p_ in blk.parameters():
            p_.requires_grad_(False)
        if adapters:
            lora.add_trainable(blk, "q,k,v,o,ffn.0,ffn.2", 32)
            with torch.no_grad():
                for _, _, ad in lora.trainable(blk):
                    ad.up[:, :32] = (torch.randn((ad.up.shape[0], 32), device=dev) / 32 ** 0.5).to(BF)
        if fp8:
            dit.enable_fp8(blk)
            for lin in (m for m in blk.modules() if isinstance(m, torch.nn.Linear)):
                dit.fp8_weight_t(lin)          # made once per weight, outside the timed region
        return blk

    def arm(blk):
        def run():
            xg = x.clone().requires_grad_(True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            with torch.enable_grad():
                tr.block_forward(blk, xg, ctx, t_mod, rope).backward(dout)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        return run
    plain = arm(block(True, False))
    arms = {"fp8 frozen": plain, "fp8 frozen + 10 adapters": arm(block(True, True)), "bf16 + 10 adapters": arm(block(False, True)),
            "fp8 frozen again": plain}
    for f in arms.values():
        f()
    ms = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, f in arms.items():
            ms[k].append(f())
    m = {k: median(v) for k, v in ms.items()}
    lora.set_beside_fp8(old[0]), tr.set_fp8_frozen(old[1]), tr.set_keep_level(old[2])
    print(f"block forward + backward, {tokens} tokens, keep level attn, rank 32: " + ", ".join(f"{k} {v:.1f} ms" for k, v in m.items())
          + f"; adapted fp8 x {m['fp8 frozen + 10 adapters'] / m['fp8 frozen']:.3f} of the frozen fp8 block, x "
          f"{m['fp8 frozen + 10 adapters'] / m['bf16 + 10 adapters']:.3f} of the bf16 adapted block", flush=True)


def step_leg(a):
    """One high-noise CFG step (cond + uncond through the expert and its ControlNet) with every block Linear attached at rank 64."""
    from goal_force_amd import dit, lora
    from goal_force_amd.pipeline import WanVideoPipeline, build_random_controlnet, build_random_expert
    dev = torch.device("cuda", 0)
    cfg = dict(dit.A14B_CONFIG)
    cfg["num_layers"] = a.layers
    n_cn = min(10, a.layers)
    mods = (build_random_expert(cfg, seed=100, device=dev), build_random_expert(cfg, seed=200, device=dev),
            build_random_controlnet(n_cn, cfg, seed=300, device=dev), build_random_controlnet(n_cn, cfg, seed=400, device=dev, zero_convs_zero=True))
    pipe = WanVideoPipeline.from_modules(*mods, device=dev)
    g = torch.Generator().manual_seed(1000)
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
    ag = torch.Generator().manual_seed(24)
    sds = []
    for m in (mods[0], mods[2]):
        sd = {}
        for name, mod in m.named_modules():
            if isinstance(mod, dit.DiTBlock):
                for lname in BLOCK_LAYERS:
                    n, k = mod.get_submodule(lname).weight.shape
                    sd[f"{name}.{lname}.lora_B.weight"] = (torch.randn((n, 64), generator=ag) / k ** 0.5).to(BF)
                    sd[f"{name}.{lname}.lora_A.weight"] = (torch.randn((64, k), generator=ag) / 8.0).to(BF)
        sds.append(sd)

    def run():
        pipe.denoise(latents, ctx_p, ctx_n, y, control, num_inference_steps=50, cfg_scale=5.0, controlnet=True, step_ids=[0], record_step_times=True)
        return pipe.last_step_ms[0][0]
    old = lora.set_beside_fp8(True)
    for m in mods:
        dit.enable_fp8(m)
    n_att = lora.attach(mods[0], sds[0], alpha=0.0) + lora.attach(mods[2], sds[1], alpha=0.0)
    modes = {"plain fp8": 0.0, "attached beside fp8": 0.7, "plain fp8 again": 0.0}
    times = {m: [] for m in modes}
    for s in modes.values():
        lora.set_strength(pipe, s)
        run()
    for _ in range(a.step_rounds):
        for m, s in modes.items():
            lora.set_strength(pipe, s)
            times[m].append(run())
    for m in mods:
        dit.enable_fp8(m, False)
    lora.set_strength(pipe, 0.7)
    run()
    times["attached on bf16"] = [run() for _ in range(a.step_rounds)]
    lora.detach(pipe)
    lora.set_beside_fp8(old)
    m = {k: median(v) for k, v in times.items()}
    print(f"CFG step, {a.layers} + {n_cn} blocks, {n_att} Linears attached at rank 64: " + ", ".join(f"{k} {v:.0f} ms" for k, v in m.items())
          + f"; attached beside fp8 x {m['attached beside fp8'] / m['plain fp8']:.3f} of plain fp8 (A/A {abs(m['plain fp8'] - m['plain fp8 again']):.0f} ms), x "
          f"{m['attached beside fp8'] / m['attached on bf16']:.3f} of bf16 attached", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", action="store_true", help="the block forward + backward arms instead of the layer arms")
    ap.add_argument("--step", action="store_true", help="the CFG-step arms instead of the layer arms")
    ap.add_argument("--layers", type=int, default=40, help="--step: blocks per expert")
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=32760)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    if a.block or a.step:
        if a.block:
            block_leg(a)
        if a.step:
            step_leg(a)
        return
    M, dev = a.tokens, "cuda"
    parent = None
    if a.parent_lib:
        import ctypes
        from goal_force_amd import _lib
        _lib.load()         # this build's library first: both then bind to the HIP runtime torch brought
        parent = ctypes.CDLL(a.parent_lib).gf_gemm_fp8
        parent.restype, parent.argtypes = _lib.BINDINGS["gf_gemm_fp8"]
    for name, N, K, epi in SHAPES:
        x = torch.randn(M, K, device=dev).to(BF)
        a8, sc = ops.quant_fp8_rowscale(x)
        w8 = ops.cast_fp8((torch.randn(N, K, device=dev) * K ** -0.5).to(BF))
        bias, gate = torch.randn(N, device=dev).to(BF), torch.randn(N, device=dev).to(BF)
        has_r = epi == ops.EPI_BIAS_GATE_RESID
        resid = torch.randn(M, N, device=dev).to(BF) if has_r else None
        out = torch.empty(M, N, device=dev, dtype=BF)
        kw = dict(epilogue=epi, resid=resid, gate=gate if has_r else None, out=out)
        for rank in RANKS:
            rp = -(-rank // 32) * 32
            down = torch.zeros(rp, K, device=dev, dtype=BF)
            down[:rank] = (torch.randn(rank, K, device=dev) * K ** -0.5).to(BF)
            up = torch.zeros(N, rp, device=dev, dtype=BF)
            up[:, :rank] = torch.randn(N, rank, device=dev).to(BF)
            t = ops.gemm(x, down)

            def two():
                with ops.options(fp8_lora_fused=False):
                    ops.gemm_fp8_lora(a8, sc, w8, bias, t, up, 0.7, **kw)
            arms = (("plain", lambda: ops.gemm_fp8(a8, sc, w8, bias, **kw)), ("two", two),
                    ("fused", lambda: ops.gemm_fp8_lora(a8, sc, w8, bias, t, up, 0.7, **kw)), ("plain_again", lambda: ops.gemm_fp8(a8, sc, w8, bias, **kw)),
                    ("t_gemm", lambda: ops.gemm(x, down)))
            if parent is not None:
                st = torch.cuda.current_stream().cuda_stream

                def plain_parent():
                    rc = parent(a8.data_ptr(), K, w8.data_ptr(), K, sc.data_ptr(), bias.data_ptr(), out.data_ptr(), N, M, N, K, int(epi),
                                resid.data_ptr() if has_r else None, N if has_r else 0, gate.data_ptr() if has_r else None, st)
                    assert rc == 0, rc
                # the parent's arm stands once behind this build's plain arm and once in front of its second timing, so that neither
                # build always follows the same neighbour (an arm behind the 0.1 ms t GEMM measured 4-6 % faster than the same kernel elsewhere)
                arms = (arms[0], ("plain_parent", plain_parent)) + arms[1:3] + (("plain_parent_again", plain_parent),) + arms[3:]
            ms = {k: [] for k, _ in arms}
            for _, f in arms:
                f()
            for _ in range(a.reps):
                for k, f in arms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.inner):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    ms[k].append(e0.elapsed_time(e1) / a.inner)
            m = {k: median(v) for k, v in ms.items()}
            aa = abs(m["plain"] - m["plain_again"])
            verdict = "fused faster than two launches by more than the A/A spread" if m["two"] - m["fused"] > aa else "NOT faster: _ok should return 0 here"
            print(f"{name} M={M} rank {rank} (pad {rp}): plain {m['plain']:.3f} ms (A/A {aa:.3f}), two launches {m['two']:.3f} (x {m['two'] / m['plain']:.2f}), "
                  f"fused {m['fused']:.3f} (x {m['fused'] / m['plain']:.2f}), t GEMM {m['t_gemm']:.3f}"
                  + (f", this build's plain {(m['plain'] + m['plain_again']) / 2:.3f} against the parent's {(m['plain_parent'] + m['plain_parent_again']) / 2:.3f} "
                     f"(its own A/A {abs(m['plain_parent'] - m['plain_parent_again']):.3f})" if parent is not None else "") + f" — {verdict}", flush=True)


if __name__ == "__main__":
    main()
