"""LoRA adapters: the reference's merge into the weights, and a reversible attached form.

* `name_dict(state_dict)` restates `GeneralLoRALoader.get_name_dict` (diffsynth/lora/__init__.py:11-26): the `lora_B` keys of a
  `lora_A` / `lora_B` file, stripped to the module names `module.named_modules()` knows.
* `load(module, state_dict, alpha)` is `GeneralLoRALoader.load` (what `WanVideoPipeline.load_lora` calls, GF:171-174): every matched
  nn.Linear gets W <- bf16(W + bf16(fp32(alpha) bf16(up down))) in place on the device (ops.lora_merge, gf_lora_merge) — the three
  bf16 roundings torch makes there.  Irreversible, and a second call stacks on the first, as in the reference.
* `attach(module, state_dict, alpha, name)` / `detach` / `set_strength`: the adapter stays beside the layer and dit.linear adds
  peft's unmerged forward, result + lora_B(lora_A(x)) * scaling, per call (ops.gemm for x down^T, ops.lora_up).  The masters are
  never written; detached or at strength 0 the layer runs its single launch again, bit for bit.  bf16 layers only — and, under
  `set_beside_fp8(True)`, enable_fp8 layers: the fp8 product plus the adapter on the bf16 input (ops.gemm_fp8_lora; VRAM:168-187).

* `add_trainable(module, target_modules, rank, alpha, name)` restates `add_lora_to_model` (src/goal_force/utils.py:450-459: peft's
  LoraConfig + inject_adapter_in_model): a TRAINABLE adapter beside every Linear peft's rule matches, `lora_A` kaiming-uniform,
  `lora_B` zero, registered under peft's parameter names.  dit.linear runs it exactly as an attached one; training.DiTBlockFn
  differentiates it (ops.lora_grad).  `trainable_state_dict` / `load_trainable_state` are the checkpoint's two directions
  (`mapping_lora_state_dict` + `load_state_dict(strict=False)`, utils.py:462-470, 577-583).

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


_BESIDE_FP8 = [False]


def set_beside_fp8(on) -> bool:
    """Open (or close) attached adapters beside enable_fp8 Linears; returns the previous setting.  Off — the default — every fp8
    combination is refused by name as ever.  On: attach / add_trainable take a Linear that carries an fp8 copy (fp4 stays refused),
    dit.linear runs the reference's AutoWrappedLinear.forward on it (VRAM:168-187) — the fp8 product of the quantised input plus the
    adapters on the bf16 input (ops.gemm_fp8_lora) — and, with training.set_fp8_frozen, the tape takes a frozen fp8 block whose only
    trainable things are live trainable adapters (dit.refuse_training).  A process-wide switch like training.set_fp8_frozen; no
    environment variable is read."""
    prev, _BESIDE_FP8[0] = _BESIDE_FP8[0], bool(on)
    return prev


def beside_fp8() -> bool:
    return _BESIDE_FP8[0]


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
    trainable = False

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


def _hosted(module):
    """What dit.linear runs: the Linears of the DiT / ControlNet blocks.  The embeddings and the head launch their GEMMs themselves
    and would never look at an adapter."""
    from . import dit
    return {id(lin) for m in module.modules() if isinstance(m, dit.LORA_HOSTS) for lin in m.modules() if isinstance(lin, nn.Linear)}


def _check_host(what, mod_name, lin, hosted, own_linears, name):
    """The layers that take an adapter beside them (attached or trainable): bf16 Linears of the blocks, one adapter per name."""
    from . import dit
    if id(lin) not in hosted and not own_linears:
        raise GoalForceError(f"{what}: {mod_name!r} is not a Linear of a DiT block (q / k / v / o, ffn.0, ffn.2), the layers an "
                             "attached adapter runs on: use the merged form (pipe.load_lora) for it")
    kind = dit.precision(lin)
    if kind != "bf16" and not (kind == "fp8" and beside_fp8()):
        raise GoalForceError(f"{what}: {mod_name!r} carries an enable_{kind} weight copy: attached adapters run on bf16 layers "
                             "only (use the merged form, pipe.load_lora, with quantised layers)")
    if any(ad.name == name for ad in adapters(lin)):
        raise GoalForceError(f"{what}: {mod_name!r} already carries an adapter named {name!r}: detach it first or choose another name")


def attach(module: nn.Module, state_dict, alpha=1.0, name="default", own_linears=False):
    """Attach every matching adapter of `state_dict` beside its Linear under `name`, at strength `alpha`.  Returns the count.
    `own_linears`: the caller runs the matched layers through dit.linear itself (a benchmark's bare nn.Linear), so layers outside
    the DiT blocks are taken too."""
    a = _alpha(alpha, "lora.attach")
    todo = plan(module, state_dict, "lora.attach")
    hosted = _hosted(module)
    for mod_name, lin, up, down in todo:
        _check_host("lora.attach", mod_name, lin, hosted, own_linears, name)
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
        for ad in hit:
            if ad.trainable:
                ad.unregister(lin)
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


# ---------------------------------------------------------------------------------------------------------------------
# trainable adapters
class _Weight(nn.Module):
    """`<linear>.lora_A.<name>` / `<linear>.lora_B.<name>`: holds `.weight`, so named_parameters() spells peft's names."""

    def __init__(self, weight):
        super().__init__()
        self.weight = nn.Parameter(weight)


class TrainableAdapter:
    """One trainable adapter of one Linear.  The parameters ARE the operands the kernels read: `lora_A.<name>.weight` [rank_pad, in]
    and `lora_B.<name>.weight` [out, rank_pad], bf16, zero beyond the true rank.  The padding has zero value and zero gradient
    (its rows of t, dt are zero), so AdamW keeps it zero, an optimiser step needs no repack, and the true-rank tensors are slices
    (trainable_state_dict).  `alpha` is the scaling lora_alpha / r that multiplies the update."""
    trainable = True

    def __init__(self, name, scaling, rank, lin, down_pad, up_pad):
        self.name, self.alpha, self.rank = name, scaling, rank
        for attr, w in (("lora_A", down_pad), ("lora_B", up_pad)):
            if not isinstance(getattr(lin, attr, None), nn.ModuleDict):
                setattr(lin, attr, nn.ModuleDict())
            getattr(lin, attr)[name] = _Weight(w)
        self._a, self._b = lin.lora_A[name], lin.lora_B[name]

    down = property(lambda self: self._a.weight)
    up = property(lambda self: self._b.weight)

    def on(self, device):
        return self                  # registered parameters move with the module

    def unregister(self, lin):
        for attr in ("lora_A", "lora_B"):
            del getattr(lin, attr)[self.name]
            if not len(getattr(lin, attr)):
                delattr(lin, attr)


def match_targets(module: nn.Module, target_modules):
    """[(name, module)] by peft's rule (tuners_utils.check_target_module_exists with a list of targets): a module is matched when
    its name equals a target or ends with "." + target.  In named_modules() order."""
    targets = [t for t in (target_modules.split(",") if isinstance(target_modules, str) else list(target_modules))]
    return [(n, m) for n, m in module.named_modules() if any(n == t or n.endswith("." + t) for t in targets)], targets


def add_trainable(module: nn.Module, target_modules, rank, alpha=None, name="default"):
    """`add_lora_to_model` (utils.py:450-459): a trainable adapter named `name` beside every Linear that peft's rule matches
    (match_targets), scaling alpha / rank with alpha = rank by default.  lora_A ~ U(-1/sqrt(in), 1/sqrt(in)) — peft's
    kaiming_uniform_(a=sqrt 5) — drawn with torch's generator in fp32 and rounded to bf16 (peft's distribution, not its draws);
    lora_B zero.  Only bf16 Linears of DiT / ControlNet blocks take one (lora.attach's rule); a target that matches nothing is an
    error by name.  Nothing else is frozen here: the caller decides what else trains.  Returns how many adapters were added."""
    from . import dit
    what = "lora.add_trainable"
    rank = int(rank)
    if not 1 <= rank <= MAX_RANK:
        raise GoalForceError(f"{what}: rank {rank}: expected 1 <= r <= {MAX_RANK}")
    scaling = _alpha(rank if alpha is None else alpha, what) / rank
    matched, targets = match_targets(module, target_modules)
    for t in targets:
        if not any(n == t or n.endswith("." + t) for n, _ in matched):
            raise GoalForceError(f"{what}: target {t!r} matches no module (peft's rule: the name equals the target or ends with '.{t}')")
    hosted = _hosted(module)
    for mod_name, lin in matched:
        if not isinstance(lin, nn.Linear):
            raise GoalForceError(f"{what}: target matches {mod_name!r}, a {type(lin).__name__}: only nn.Linear layers take an adapter")
        _check_host(what, mod_name, lin, hosted, False, name)
        w = lin.weight
        if w.dtype != torch.bfloat16:
            raise GoalForceError(f"{what}: {mod_name!r}: the weight must be bf16, got {w.dtype}")
        if w.shape[0] % 64 or w.shape[1] % 64:       # x down^T and dy up sum over them on the GEMM (its K step)
            raise GoalForceError(f"{what}: {mod_name!r} is {tuple(w.shape)}: a trainable adapter takes features that are multiples of 64")
        # under set_beside_fp8 the layer may get its fp8 copy after this call (scripts/train.py: add_lora, then enable_fp8_training):
        # asked whatever the layer's precision is now.  dX = dY W8 sums over out_features on the fp8 GEMM, whose K step is 128.
        if beside_fp8() and (w.shape[0] % 128 or w.shape[1] % 128):
            raise GoalForceError(f"{what}: {mod_name!r} is {tuple(w.shape)}: under lora.set_beside_fp8 a trainable adapter takes features "
                                 "that are multiples of 128 (the fp8 GEMMs' K step, forward and dX)")
    rp = -(-rank // RANK_TILE) * RANK_TILE
    for mod_name, lin in matched:
        n_out, k_in = lin.weight.shape
        dev = lin.weight.device
        down = torch.zeros((rp, k_in), dtype=torch.bfloat16)
        bound = 1.0 / math.sqrt(k_in)
        down[:rank] = torch.empty((rank, k_in), dtype=torch.float32).uniform_(-bound, bound).to(torch.bfloat16)
        ads = list(adapters(lin))
        ads.append(TrainableAdapter(name, scaling, rank, lin, down.to(dev), torch.zeros((n_out, rp), dtype=torch.bfloat16, device=dev)))
        lin._gf_lora = ads
    if matched:
        _changed()
    return len(matched)


def trainable(module: nn.Module):
    """[(linear's name, the Linear, adapter)] of every trainable adapter inside `module`, in named_modules() and attach order."""
    return [(n, m, ad) for n, m in module.named_modules() for ad in adapters(m) if ad.trainable]


def trainable_parameters(module: nn.Module):
    """The parameters of the trainable adapters inside `module` (lora_A then lora_B per adapter)."""
    return [p for _, _, ad in trainable(module) for p in (ad.down, ad.up)]


def trainable_state_dict(module: nn.Module, prefix=""):
    """{prefix + "<linear>.lora_A.<name>.weight": [r, in], ... "lora_B.<name>.weight": [out, r]}: the true-rank tensors under peft's
    names (the padding is cut off), detached copies on the parameters' device."""
    out = {}
    for n, _, ad in trainable(module):
        dot = n + "." if n else ""
        out[f"{prefix}{dot}lora_A.{ad.name}.weight"] = ad.down.detach()[:ad.rank].clone()
        out[f"{prefix}{dot}lora_B.{ad.name}.weight"] = ad.up.detach()[:, :ad.rank].clone()
    return out


def load_trainable_state(module: nn.Module, state_dict, source=None):
    """`mapping_lora_state_dict` + `load_state_dict(strict=False)` (utils.py:462-470, 577-583): keys spelt `lora_A.weight` /
    `lora_B.weight` are read as the adapter "default", `lora_A.default.weight` / `lora_B.default.weight` as they are, every other
    key is dropped; a mapped key that names no trainable adapter is reported as the reference reports it, a trainable adapter the
    file does not name keeps its initial values, a tensor of another shape is an error (as load_state_dict makes it one).  Returns
    (number of tensors loaded, unexpected keys)."""
    mapped = {}
    for key, value in state_dict.items():
        if "lora_A.weight" in key or "lora_B.weight" in key:
            mapped[key.replace("lora_A.weight", "lora_A.default.weight").replace("lora_B.weight", "lora_B.default.weight")] = value
        elif "lora_A.default.weight" in key or "lora_B.default.weight" in key:
            mapped[key] = value
    slots = {}
    for n, _, ad in trainable(module):
        dot = n + "." if n else ""
        slots[f"{dot}lora_A.{ad.name}.weight"] = (ad.down, (ad.rank, ad.down.shape[1]), (slice(0, ad.rank), slice(None)))
        slots[f"{dot}lora_B.{ad.name}.weight"] = (ad.up, (ad.up.shape[0], ad.rank), (slice(None), slice(0, ad.rank)))
    unexpected = [k for k in mapped if k not in slots]
    for key, value in mapped.items():
        if key in slots and tuple(value.shape) != slots[key][1]:
            raise GoalForceError(f"lora.load_trainable_state: {key!r} is {tuple(value.shape)}, the adapter holds {slots[key][1]}")
    n = 0
    with torch.no_grad():
        for key, value in mapped.items():
            if key in slots:
                p, _, at = slots[key]
                p[at] = value.detach().to(device=p.device, dtype=p.dtype)
                n += 1
    if source is not None:
        print(f"LoRA checkpoint loaded: {source}, total {len(mapped)} keys")
    if unexpected:
        print(f"Warning, LoRA key mismatch! Unexpected keys in LoRA checkpoint: {unexpected}")
    if n:
        _changed()
    return n, unexpected
