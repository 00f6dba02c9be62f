"""Generates tests/golden/g21_lora.npz by RUNNING THE REFERENCE's own `GeneralLoRALoader` (diffsynth/lora/__init__.py; build container
only, like make_goldens.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_lora_golden.py

The reference's WanModel at the tiny width of g5, in bf16 on the CPU, takes the two adapter files of tests/lora_refs.GOLDEN_LOADS one
after the other (the second stacks on the first) through `GeneralLoRALoader(device="cpu", torch_dtype=bf16).load(model, file, alpha)`,
in two data classes: small integers (every sum exact in any order) and Gaussian operands.  The files spell the keys both ways
(`lora_B.weight` / `lora_B.default.weight`, with and without `diffusion_model.`), carry keys that match nothing, ranks 4 and 33,
alpha 1 and 0.7, adapters on q / k / v / o of both attentions, ffn.0, ffn.2, text_embedding.0 and head.head.

Stored (data only): the files' key lists and the dictionaries `get_name_dict` made of them (JSON), the update counts the loader printed,
and per class, load and layer the sha256 of the reference's merged weight together with the (few) elements where it differs from the
exact chain of tests/lora_refs.py — position and the reference's bits.  The tests rebuild the reference's tensor from the seeded
inputs, the chain and that list, and the sha256 proves the rebuilt tensor to be the reference's bit for bit: the whole result at a
few kilobytes.

The run ASSERTS what keeps the comparison meaningful: on integers the reference equals the chain on every element; on gauss it
differs on at most 2^-12 of the elements of any layer, by one bf16 step where it does.  The CPU figure is stored."""
import contextlib
import importlib.util
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_goldens as mg  # noqa: E402  (imports _ref_import, disables grad)
import lora_refs as LR  # noqa: E402
from forward_refs import bf16_steps, bits  # noqa: E402

BF = torch.bfloat16
SHARE_CAP = 2.0 ** -12


def reference_loader():
    """The real diffsynth/lora/__init__.py (_ref_import registers a stub under that name for the pipeline module's import)."""
    spec = importlib.util.spec_from_file_location("gf_ref_lora", os.path.join(mg._ref_import.REF, "diffsynth", "lora", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.GeneralLoRALoader


def main():
    ref = mg._ref_import.load_reference(with_dataset=False)
    Loader = reference_loader()
    out = {}
    worst = 0.0
    for cls in LR.GOLDEN_CLASSES:
        dit = mg._build_tiny_models(ref, False, BF)[0]
        base = LR.golden_base_sd(cls)
        dit.load_state_dict(base, strict=True)
        modules = dict(dit.named_modules())
        for load, (_, _, r, alpha) in enumerate(LR.GOLDEN_LOADS):
            lsd = LR.golden_lora_sd(load, cls, base)
            loader = Loader(device="cpu", torch_dtype=BF)
            names = loader.get_name_dict(lsd)
            said = io.StringIO()
            with contextlib.redirect_stdout(said):
                loader.load(dit, lsd, alpha=alpha)
            n_updated = int(said.getvalue().split()[0])
            assert said.getvalue().strip() == f"{n_updated} tensors are updated by LoRA." and n_updated == len(LR.GOLDEN_TARGETS)
            assert sorted(n for n in names if n in modules) == sorted(LR.GOLDEN_TARGETS)
            out[f"keys_{load}"] = np.array(json.dumps(list(lsd)))
            out[f"name_dict_{load}"] = np.array(json.dumps(names))
            out[f"updated_{load}"] = np.array(n_updated)
            hit = {n: names[n] for n in LR.GOLDEN_TARGETS}
            chain = LR.merged_state(base, lsd, hit, alpha)
            base = dict(base)
            for i, n in enumerate(LR.GOLDEN_TARGETS):
                got, want = modules[n].weight.detach().clone(), chain[n + ".weight"]
                diff = bits(got) != bits(want)
                share = float(diff.double().mean())
                steps = int(bf16_steps(got, want).max())
                worst = max(worst, share)
                if cls == "integers":
                    assert not bool(diff.any()), f"{cls} load {load} {n}: the reference differs from the exact chain on exact operands"
                else:
                    assert share <= SHARE_CAP and steps <= 1, f"{cls} load {load} {n}: share {share:.2e}, {steps} steps"
                idx = torch.nonzero(diff.reshape(-1)).reshape(-1)
                out[f"{cls}_{load}_{i}_idx"] = idx.numpy().astype(np.int32)
                out[f"{cls}_{load}_{i}_val"] = bits(got).reshape(-1)[idx].numpy()
                out[f"{cls}_{load}_{i}_sha"] = np.array(LR.sha(got))
                base[n + ".weight"] = got
            print(f"{cls} load {load} (rank {r}, alpha {alpha}): {n_updated} updated; worst share so far {worst:.2e}", flush=True)
    out["cpu_share"] = np.array(worst)
    out["share_cap"] = np.array(SHARE_CAP)
    mg.save("g21_lora.npz", **out)


if __name__ == "__main__":
    main()
