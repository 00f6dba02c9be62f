"""Production-size drift of the SageAttention backend (profiles/r08): ONE noise prediction (step 0 of the 50-step schedule, cond
branch, high-noise expert with its ControlNet, 40 + 10 blocks, 32760 tokens, the random weights of tests/fullsize_parity.py) with
dit.enable_sage_attention on and off, each against the fp32 arithmetic of the oracle on the same GPU — the number DESIGN §6 reports
for the bf16 path (1.74e-2).  With --fp8 the same with fp8 linears (config 5).  One JSON line.

  python tools/sage_drift.py [--fp8]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fullsize_parity as fp  # noqa: E402
from goal_force_amd.dit import enable_fp8, enable_sage_attention  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fp8", action="store_true")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda", torch.cuda.current_device())
    t0 = time.time()
    cfg, pipe = fp.build(40, 10, dev, need_low=False)
    fp.make_peaky(pipe)
    inp = fp.inputs(pipe, (21, 60, 104), dev)
    pipe.scheduler.set_timesteps(50, shift=5.0)
    ts = pipe.scheduler.timesteps[0].unsqueeze(0).to(dtype=torch.bfloat16, device=dev)
    outs = {}
    for f8 in ((False, True) if a.fp8 else (False,)):
        for m in (pipe.dit, pipe.controlnet):
            enable_fp8(m, f8)
        for sage in (False, True):
            for m in (pipe.dit, pipe.controlnet):
                enable_sage_attention(m, sage)
            outs[f"{'fp8' if f8 else 'bf16'}_{'sage' if sage else 'k3'}"] = fp.hip_forward(pipe, inp, ts, ())[0].float()
    for m in (pipe.dit, pipe.controlnet):
        enable_fp8(m, False)
        enable_sage_attention(m, False)
    ref = fp.OracleRunner(pipe, cfg, torch.float32).forward(0, inp["latents"].float(), ts, inp["ctx_p"], inp)
    torch.cuda.synchronize()
    rep = {"what": "noise prediction, step 0 cond, 40 + 10 blocks, 32760 tokens, rel-L2 against the fp32 oracle",
           "device": torch.cuda.get_device_name(0), "wall_s": None}
    rep.update({k: fp.rel_l2(v, ref) for k, v in outs.items()})
    rep["wall_s"] = time.time() - t0
    print(json.dumps(rep))


if __name__ == "__main__":
    main()
