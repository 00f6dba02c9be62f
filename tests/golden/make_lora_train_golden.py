#!/usr/bin/env python3
"""g22: four LoRA training steps on the tiny expert, restated in torch on the CPU — the oracle's model_fn (oracle/wan_oracle.py, pinned
to the reference's by g5) with peft's unmerged forward on every block Linear,

    result = result + lora_B(lora_A(x)) * scaling            (peft/tuners/lora/layer.py, Linear.forward; dropout off, scaling alpha / r = 1)

the reference's training_loss (oracle/train_oracle.py, pinned by g9), torch.optim.AdamW over lora_A / lora_B only, ConstantLR with
torch's defaults and clip_grad_norm_, as launch_training_task drives them (utils.py:755-810).  peft itself is not installed in this
image: the three lines above are its forward, the rest is the reference's own arithmetic as the oracle restates it.  Two runs, fp32
and bf16 (parameters, moments and activations in the run's dtype, as the reference trains), with the same fixed latents, noise and
timesteps per step.  Writes tests/golden/g22_lora_train.npz: per-step loss and pre-clip gradient norm of both runs, learning rates.

    python tests/golden/make_lora_train_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]

import gen_inputs as gi  # noqa: E402
import lora_train_refs as T  # noqa: E402
from oracle import train_oracle as to  # noqa: E402
from oracle import wan_oracle as wo  # noqa: E402


def run(dtype):
    cfg = dict(gi.TINY)
    sd0 = gi.dit_sd(cfg, seed=41)
    sd = {k: v.detach().to(dtype) for k, v in sd0.items()}
    lo = {n: (torch.nn.Parameter(a.to(dtype)), torch.nn.Parameter(b.to(dtype))) for n, (a, b) in T.loop_adapters(cfg, sd0).items()}
    params = [p for ab in lo.values() for p in ab]
    opt = torch.optim.AdamW(params, lr=T.LOOP["learning_rate"], weight_decay=T.LOOP["weight_decay"])
    sched = torch.optim.lr_scheduler.ConstantLR(opt)
    inp = {k: v.to(dtype) for k, v in gi.train_inputs().items()}
    plain = wo._lin

    def lin(x, sd_, name):
        y = plain(x, sd_, name)
        if name in lo:
            a, b = lo[name]
            y = y + torch.nn.functional.linear(torch.nn.functional.linear(x, a), b) * 1.0
        return y

    rec = dict(loss=[], grad_norm=[], lr=[])
    wo._lin = lin
    try:
        for step in range(T.LOOP["steps"]):
            opt.zero_grad()
            with torch.enable_grad():
                loss = to.training_loss(sd, None, cfg, 0, inp["input_latents"], inp["noise"], inp["context"], inp["y"], None,
                                        T.LOOP["timestep_ids"][step], timestep_dtype=torch.bfloat16)
                loss.backward()
            rec["lr"].append(opt.param_groups[0]["lr"])
            rec["grad_norm"].append(float(torch.nn.utils.clip_grad_norm_(params, T.LOOP["max_grad_norm"])))
            opt.step()
            sched.step()
            rec["loss"].append(float(loss.detach()))
    finally:
        wo._lin = plain
    return rec


def main():
    torch.manual_seed(0)
    f32, b16 = run(torch.float32), run(torch.bfloat16)
    assert f32["lr"] == b16["lr"]
    out = os.path.join(HERE, "g22_lora_train.npz")
    np.savez(out, loss_f32=np.array(f32["loss"]), loss_bf16=np.array(b16["loss"]), grad_norm_f32=np.array(f32["grad_norm"]),
             grad_norm_bf16=np.array(b16["grad_norm"]), lr=np.array(f32["lr"]), timestep_ids=np.array(T.LOOP["timestep_ids"]))
    print("fp32 ", f32)
    print("bf16 ", b16)
    print("wrote", out)


if __name__ == "__main__":
    main()
