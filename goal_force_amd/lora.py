"""LoRA adapters: the reference's merge into the weights, and a reversible attached form.

* `name_dict(state_dict)` restates `GeneralLoRALoader.get_name_dict` (diffsynth/lora/__init__.py:11-26): the `lora_B` keys of a
  `lora_A` / `lora_B` file, stripped to the module names `module.named_modules()` knows.
* `load(module, state_dict, alpha)` is `GeneralLoRALoader.load` (what `WanVideoPipeline.load_lora` calls, GF:171-174): every matched
  nn.Linear gets W <- bf16(W + bf16(fp32(alpha) bf16(up down))) in place on the device (ops.lora_merge, gf_lora_merge) — the three
  bf16 roundings torch makes there.  Irreversible, and a second call stacks on the first, as in the reference.
* `attach(module, state_dict, alpha, name)` / `detach` / `set_strength`: the adapter stays beside the layer and dit.linear adds
  peft's unmerged forward, result + lora_B(lora_A(x)) * scaling, per call (ops.gemm for x down^T, ops.lora_up).  The masters are
  never written; detached or at strength 0 the layer runs its single launch again, bit for bit.  bf16 layers only.

Every refusal names the key or the module and comes before the first weight is touched.  The kohya spelling (`lora_up` /
`lora_down` / `.alpha`) is not what the reference's loader reads: such a file matches nothing and 0 updates are reported, as there.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import ops
from ._lib import GoalForceError

MAX_RANK = 256       # gf_lora_merge / gf_lora_up
RANK_TILE = 32       # attach pads the rank to a multiple of this (one MFMA's K; it also gives ops.gemm its N % 8)


def name_dict(state_dict):
    """{module name: (lora_B key, lora_A key)} — GeneralLoRALoader.get_name_dict: only keys that contain `.lora_B.`; the adapter
    name after `lora_B` (`lora_B.default.weight`) is optional; a leading `diffusion_model.` and the trailing `weight` are dropped."""
    out = {}
    for key in state_dict:
        if ".lora_B." not in key:
            continue
        keys = key.split(".")
        at = keys.index("lora_B")
        if len(keys) > at + 2:
            keys.pop(at + 1)
        keys.pop(at)
        if keys[0] == "diffusion_model":
            keys.pop(0)
        keys.pop(-1)
        out[".".join(keys)] = (key, key.replace(".lora_B.", ".lora_A."))
    return out


def _alpha(alpha, what):
    try:
        a = float(alpha)
    except (TypeError, ValueError) as e:
        raise GoalForceError(f"{what}: alpha must be a number, got {alpha!r}") from e
    if not math.isfinite(a):
        raise GoalForceError(f"{what}: alpha must be finite, got {alpha!r}")
    return a


def plan(module: nn.Module, state_dict, what="lora"):
    """[(module name, the nn.Linear, up [out, r], down [r, in])] of the adapters in `state_dict` that match a module of `module`,
    in named_modules() order, checked: nothing is converted, moved or written here."""
    names = name_dict(state_dict)
    out = []
    for name, m in module.named_modules():
        if name not in names:
            continue
        key_b, key_a = names[name]
        if key_a not in state_dict:         # (asked of matched names only: a key that matches no module is ignored whole, as in the reference)
            raise GoalForceError(f"{what}: {key_b!r} has no partner {key_a!r}")
        up, down = state_dict[key_b], state_dict[key_a]
        if not isinstance(m, nn.Linear):
            raise GoalForceError(f"{what}: {key_b!r} addresses {name!r}, a {type(m).__name__}: only nn.Linear layers take an adapter")
        if up.dim() != 2 or down.dim() != 2:
            raise GoalForceError(f"{what}: {key_b!r} / {key_a!r} must be 2-D (Conv adapters are outside this project), got "
                                 f"{tuple(up.shape)} / {tuple(down.shape)}")
        n_out, k_in = m.weight.shape
        r = up.shape[1]
        if up.shape[0] != n_out or down.shape != (r, k_in):
            raise GoalForceError(f"{what}: {name!r} is [{n_out}, {k_in}]: expected {key_b!r} [{n_out}, r] and {key_a!r} [r, {k_in}], got "
                                 f"{tuple(up.shape)} and {tuple(down.shape)}")
        if not 1 <= r <= MAX_RANK:
            raise GoalForceError(f"{what}: {key_b!r} has rank {r}: expected 1 <= r <= {MAX_RANK}")
        out.append((name, m, up, down))
    return out


def _report(n):
    print(f"{n} tensors are updated by LoRA.")
    return n


def load(module: nn.Module, state_dict, alpha=1.0):
    """GeneralLoRALoader.load: merge every matching adapter into its Linear's weight, in place (see the module's words).  Returns
    the number of updated tensors and prints the reference's line.  Every copy derived from the weights (fp8 / fp4 copies, the
    padded patch weight, the cross-attention's fold tables, cached context projections) follows on its own."""
    from . import dit
    a = _alpha(alpha, "load_lora")
    todo = plan(module, state_dict, "load_lora")
    for name, lin, up, down in todo:
        w = lin.weight
        if not w.is_cuda or w.dtype != torch.bfloat16:
            raise GoalForceError(f"load_lora: {name!r}: the weight must be bf16 on the GPU (no CPU fallback exists), got {w.dtype} on {w.device}")
        # what gf_lora_merge would refuse, asked here of every layer before the first one is written
        if w.dim() != 2 or w.stride(1) != 1 or w.shape[1] % 8 or w.stride(0) % 8 or w.data_ptr() % 16:
            raise GoalForceError(f"load_lora: {name!r}: gf_lora_merge takes a weight with contiguous rows, in_features and row pitch multiples "
                                 f"of 8 and a 16-byte aligned base, got {tuple(w.shape)} with strides {tuple(w.stride())}")
    for name, lin, up, down in todo:
        w = lin.weight
        ops.lora_merge(w, up.detach().to(device=w.device, dtype=torch.bfloat16).contiguous(),
                       down.detach().to(device=w.device, dtype=torch.bfloat16).contiguous(), a)
    if todo:
        dit.invalidate_caches()      # (inference tensors carry no version counter for ops.lora_merge to bump)
    return _report(len(todo))


class Adapter:
    """One attached adapter of one Linear: `down` [rank_pad, in] and `up` [out, rank_pad] bf16, zero beyond the true rank."""
    __slots__ = ("name", "alpha", "rank", "down", "up")

    def __init__(self, name, alpha, up, down, device):
        r = up.shape[1]
        rp = -(-r // RANK_TILE) * RANK_TILE
        self.name, self.alpha, self.rank = name, alpha, r
        self.down = torch.zeros((rp, down.shape[1]), dtype=torch.bfloat16, device=device)
        self.up = torch.zeros((up.shape[0], rp), dtype=torch.bfloat16, device=device)
        self.down[:r] = down.detach().to(device=device, dtype=torch.bfloat16)
        self.up[:, :r] = up.detach().to(device=device, dtype=torch.bfloat16)

    def on(self, device):
        """The operands on `device` (a module moved after attach is followed once)."""
        if self.down.device != device:
            self.down, self.up = self.down.to(device), self.up.to(device)
        return self


def adapters(lin: nn.Module):
    """Every adapter attached to the layer, in attach order."""
    return getattr(lin, "_gf_lora", ())


def live(lin: nn.Module):
    """The adapters dit.linear applies: those of non-zero strength, in attach order."""
    ads = getattr(lin, "_gf_lora", None)
    return [a for a in ads if a.alpha != 0.0] if ads else ()


def _changed():
    from . import dit
    dit.invalidate_caches()          # no ContextCache entry or fold table outlives the change


def attach(module: nn.Module, state_dict, alpha=1.0, name="default", own_linears=False):
    """Attach every matching adapter of `state_dict` beside its Linear under `name`, at strength `alpha`.  Returns the count.
    `own_linears`: the caller runs the matched layers through dit.linear itself (a benchmark's bare nn.Linear), so layers outside
    the DiT blocks are taken too."""
    from . import dit
    a = _alpha(alpha, "lora.attach")
    todo = plan(module, state_dict, "lora.attach")
    # what dit.linear runs: the Linears of the DiT / ControlNet blocks.  The embeddings and the head launch their GEMMs themselves
    # and would never look at an adapter
    hosted = {id(lin) for m in module.modules() if isinstance(m, dit.LORA_HOSTS) for lin in m.modules() if isinstance(lin, nn.Linear)}
    for mod_name, lin, up, down in todo:
        if id(lin) not in hosted and not own_linears:
            raise GoalForceError(f"lora.attach: {mod_name!r} is not a Linear of a DiT block (q / k / v / o, ffn.0, ffn.2), the layers an "
                                 "attached adapter runs on: use the merged form (pipe.load_lora) for it")
        kind = dit.precision(lin)
        if kind != "bf16":
            raise GoalForceError(f"lora.attach: {mod_name!r} carries an enable_{kind} weight copy: attached adapters run on bf16 layers "
                                 "only (use the merged form, pipe.load_lora, with quantised layers)")
        if any(ad.name == name for ad in adapters(lin)):
            raise GoalForceError(f"lora.attach: {mod_name!r} already carries an adapter named {name!r}: detach it first or choose another name")
    for mod_name, lin, up, down in todo:
        ads = list(adapters(lin))
        ads.append(Adapter(name, a, up, down, lin.weight.device))
        lin._gf_lora = ads
    if todo:
        _changed()
    return len(todo)


def _named(module, name):
    for lin in module.modules():
        ads = getattr(lin, "_gf_lora", None)
        if ads:
            yield lin, [ad for ad in ads if name is None or ad.name == name]


def detach(module: nn.Module, name=None):
    """Remove the adapters called `name` (None: all) from every layer inside `module`.  Returns how many were removed."""
    n = 0
    for lin, hit in list(_named(module, name)):
        n += len(hit)
        rest = [ad for ad in lin._gf_lora if not any(ad is h for h in hit)]
        if rest:
            lin._gf_lora = rest
        else:
            del lin._gf_lora
    if n:
        _changed()
    return n


def set_strength(module: nn.Module, alpha, name=None):
    """Set the strength of the adapters called `name` (None: all) inside `module`; 0 switches them off.  Returns how many."""
    a = _alpha(alpha, "lora.set_strength")
    n = 0
    for _, hit in _named(module, name):
        for ad in hit:
            ad.alpha = a
            n += 1
    if n:
        _changed()
    return n
