"""Wan DiT (Wan2.2-I2V-A14B expert) — host-side mirror of the reference's module interface with
every forward implemented by the HIP kernels in libgoalforce_hip.so.

Drop-in surface: class names, constructor arguments, forward signatures and
state_dict key names follow diffsynth/models/wan_video_dit.py (DIT) so reference checkpoints load
unchanged (`blocks.N.self_attn.q.weight`, ..., DIT:273-340).  The nn.Linear / nn.LayerNorm
submodules are parameter containers only — their torch forwards are never called.

Activations are token-major [S, D] bf16 (batch 1 per call on the hot path; B > 1 is looped).
"""
from __future__ import annotations

import functools
import math
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import lora, ops
from ._lib import GoalForceError


# ------------------------------------------------------------------ RoPE tables (host, fp64 -> fp32)
def precompute_freqs_cis(dim: int, end: int = 1024, theta: float = 10000.0):
    """DIT:83-89 — complex128 table [end, dim/2]."""
    freqs = 1.0 / (theta ** (torch.arange(0, dim, 2)[: (dim // 2)].double() / dim))
    freqs = torch.outer(torch.arange(end), freqs)
    return torch.polar(torch.ones_like(freqs), freqs)


def precompute_freqs_cis_3d(dim: int, end: int = 1024, theta: float = 10000.0):
    """DIT:75-80 — (frame, height, width) tables; pairs split (d-2(d//3))/2, (d//3)/2, (d//3)/2."""
    return (precompute_freqs_cis(dim - 2 * (dim // 3), end, theta),
            precompute_freqs_cis(dim // 3, end, theta),
            precompute_freqs_cis(dim // 3, end, theta))


class RopeTable:
    """cos/sin of the per-token rotary phases, resident in HBM as fp32 [S, head_dim/2] each.
    Built once per (f, h, w) grid instead of the reference's per-forward CPU rebuild + H2D copy
    (GF:1474-1478)."""

    def __init__(self, freqs_complex: torch.Tensor, device, grid=None):
        fc = freqs_complex.reshape(freqs_complex.shape[0], -1)
        self.grid = grid                  # the (f, h, w) token grid when the table was built from one (sparse attention patterns ask for it)
        self.cos = fc.real.to(torch.float32).contiguous().to(device)
        self.sin = fc.imag.to(torch.float32).contiguous().to(device)
        self.tokens = fc.shape[0]
        self._scaled = {}

    def scaled(self, c: float):
        """(c cos, c sin): the rotation that also multiplies by c.  The self-attention's Q goes through it with c = softmax scale x
        log2(e) (SelfAttention.attend), so that the attention kernel's operand Q' = bf16(c q) is produced from the fp32 rotation with
        ONE rounding — where rounding q to bf16 first and c q again (what the kernel does to a plain q) costs the logits a second one."""
        tabs = self.__dict__.setdefault("_scaled", {})          # (shard tables are built without __init__: sequence_parallel.shard_rope)
        if c not in tabs:
            tabs[c] = ((self.cos * c).contiguous(), (self.sin * c).contiguous())
        return tabs[c]

    @staticmethod
    def from_grid(freqs3: Tuple[torch.Tensor, torch.Tensor, torch.Tensor], f: int, h: int, w: int, device):
        tab = torch.cat([
            freqs3[0][:f].view(f, 1, 1, -1).expand(f, h, w, -1),
            freqs3[1][:h].view(1, h, 1, -1).expand(f, h, w, -1),
            freqs3[2][:w].view(1, 1, w, -1).expand(f, h, w, -1),
        ], dim=-1).reshape(f * h * w, -1)
        return RopeTable(tab, device, grid=(f, h, w))


def Q_PRESCALE(head_dim: int) -> float:
    """c = fp32(fp32(1 / sqrt(head_dim)) x fp32(log2 e)) — bit for bit the factor the attention launcher folds into Q (gf_attention.hip:
    `scale_log2e = scale * 1.4426950408889634f`)."""
    import numpy as np
    return float(np.float32(np.float32(1.0 / math.sqrt(head_dim)) * np.float32(1.4426950408889634)))


def _as_rope(freqs, device) -> RopeTable:
    if isinstance(freqs, RopeTable):
        return freqs
    if torch.is_tensor(freqs) and freqs.is_complex():  # the reference's [S,1,d/2] complex table
        return RopeTable(freqs.detach().cpu(), device)
    raise GoalForceError("freqs must be a RopeTable or the reference's complex [S,1,d/2] tensor")


_SINUSOID_FREQS = {}


def sinusoidal_embedding_1d(dim, position):
    """DIT:68-72: cat(cos, sin)(t * 10000^(-i/(dim/2))) in fp64, cast to position.dtype.  The frequency table is built once
    on the host (the reference's fp64 `pow`) and kept on the timestep's device; the product, cos and sin run there in
    fp64 too, so a forward no longer pulls the timestep to the host (a hidden D2H sync, 100 x per video)."""
    key = (dim, position.device)
    inv = _SINUSOID_FREQS.get(key)
    if inv is None:
        inv = torch.pow(10000, -torch.arange(dim // 2, dtype=torch.float64).div(dim // 2)).to(position.device)
        _SINUSOID_FREQS[key] = inv
    sinusoid = torch.outer(position.detach().type(torch.float64), inv)
    return torch.cat([torch.cos(sinusoid), torch.sin(sinusoid)], dim=1).to(position.dtype)


# ------------------------------------------------------------------ B3: the reference's module-level functions (DIT:28, 64, 92)
def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int, compatibility_mode=False):
    """DIT:28-61 — q, k, v [B, S, num_heads * head_dim] (`b s (n d)`) -> [B, Sq, num_heads * head_dim]: softmax(q k^T / sqrt(d)) v
    per head, no mask, on the HIP flash-attention kernels (gf_flash_attn_fwd).  `compatibility_mode` only chooses among the
    reference's backends (flash-attn 3 / 2, sageattention, torch SDPA) and is accepted and ignored here; the sageattention branch is
    `sageattn` below (bound into the reference) and `enable_sage_attention` for the package's own blocks.
    The q handed in is final (already rounded to bf16 by its producer), so long key sequences run on the kernel that scales the fp32
    scores — SDPA's precision at peaky logits — not on the one that pre-scales and re-rounds Q (ops.flash_attn: finished_q); the
    package's own blocks produce a pre-scaled q instead and keep the faster kernel (SelfAttention.attend)."""
    if q.dim() != 3 or k.dim() != 3 or v.dim() != 3 or not (q.shape[0] == k.shape[0] == v.shape[0]):
        raise GoalForceError("flash_attention: q, k, v must be [B, S, num_heads * head_dim] with equal B")
    return torch.stack([ops.flash_attn(q[b].contiguous(), k[b].contiguous(), v[b].contiguous(), num_heads, finished_q=True)
                        for b in range(q.shape[0])])


def modulate(x: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor):
    """DIT:64-65 — x * (1 + scale) + shift with x [B, S, D] and shift / scale broadcastable [B or 1, 1, D] (or [D]), computed in
    the reference's eager bf16 rounding sequence by gf_modulate."""
    if x.dim() == 2:
        return ops.modulate(x, shift.reshape(-1).contiguous(), scale.reshape(-1).contiguous())
    d = x.shape[-1]
    sh, sc = (t.reshape(-1, d) if t.numel() != d else t.reshape(1, d) for t in (shift, scale))
    if sh.shape[0] not in (1, x.shape[0]) or sc.shape[0] not in (1, x.shape[0]):
        raise GoalForceError("modulate: shift / scale must be [B or 1, 1, D] (per-token modulation is outside the Goal-Force path)")
    return torch.stack([ops.modulate(x[b].contiguous(), sh[b if sh.shape[0] > 1 else 0].contiguous(),
                                     sc[b if sc.shape[0] > 1 else 0].contiguous()) for b in range(x.shape[0])])


def rope_apply(x: torch.Tensor, freqs, num_heads: int):
    """DIT:92-97 — x [B, S, num_heads * head_dim], freqs the reference's complex [S, 1, head_dim / 2] table (or a RopeTable):
    adjacent pairs of every head rotated by the token's phases (gf_rope_apply, fp32 math, one rounding to bf16)."""
    rope = _as_rope(freqs, x.device)
    hd = x.shape[-1] // num_heads
    return torch.stack([ops.rope_apply(x[b].contiguous(), rope.cos, rope.sin, hd) for b in range(x.shape[0])])


_CACHE_EPOCH = [0]


def invalidate_caches():
    """Every copy derived from a parameter (K-padded patch weights, fp8 weight copies, the ControlNet's all-zero flag, memoised
    context projections) is rebuilt on its next use.  Needed only for changes param_key cannot see: a raw-pointer write to a
    weight, or an in-place edit of an inference tensor."""
    _CACHE_EPOCH[0] += 1


def param_key(*tensors):
    """Identity + modification state of parameters a derived copy was built from: (object id, device, storage address, autograd
    version) per tensor.  Optimiser steps (ops.adamw_step bumps the version), load_state_dict, .to() and in-place edits all change
    it, so a cache that compares keys can never serve weights captured before an update.  Inference tensors (a pipeline built
    under torch.inference_mode()) carry no version counter — reading `_version` raises there — so their key is identity +
    address only: after an in-place edit of such a weight (or a raw-pointer write to any weight) call `invalidate_caches()`,
    the hook for changes the key cannot see."""
    return (_CACHE_EPOCH[0],) + tuple((id(t), str(t.device), t.data_ptr(), None if t.is_inference() else t._version) for t in tensors)


# A Linear's low-precision modes, the one that wins first: kind -> (the attribute of its weight copy, whose master's param_key is in
# <attribute>_key; the ops quantiser of a weight; of an activation; the LayerNorm producing the activation), looked up at call time
_QUANT = {"fp4": ("_gf_w4", "quant_mxfp4", "quant_mxfp4", "layernorm_modulate_mxfp4"),
          "fp8": ("_gf_w8", "cast_fp8", "quant_fp8_rowscale", "layernorm_modulate_fp8")}


def precision(lin: nn.Module, kinds=tuple(_QUANT)) -> str:
    """"fp4" | "fp8" | "bf16": the first of `kinds` the layer carries a weight copy of — what dit.linear runs it in."""
    return next((k for k in kinds if getattr(lin, _QUANT[k][0], None) is not None), "bf16")


def weight_copy(lin: nn.Linear, kind: str, enabled=None):
    """The layer's copy of `kind`, quantised again if the bf16 master changed since (param_key), or None; `enabled`: make / remove it."""
    attr, quantise = _QUANT[kind][:2]
    copy = getattr(lin, attr, None)
    if enabled is not None or (copy is not None and getattr(lin, attr + "_key") != param_key(lin.weight)):
        copy = None if enabled is False else getattr(ops, quantise)(lin.weight.detach().contiguous())
        setattr(lin, attr, copy)
        setattr(lin, attr + "_key", None if copy is None else param_key(lin.weight))
    return copy


fp8_weight = functools.partial(weight_copy, kind="fp8")    # the layer's current e4m3 copy (enable_fp8), or None
fp4_weight = functools.partial(weight_copy, kind="fp4")    # ... MXFP4 copy (enable_fp4) as (packed e2m1 codes, E8M0 scales), or None


def fp8_weight_t(lin: nn.Linear):
    """The transposed e4m3 copy `_gf_w8t` [in_features, out_features] of an enable_fp8 layer (ops.cast_fp8_t): the weight operand of
    dX = dY · W8 on ops.gemm_fp8 (training.linear_dx_fp8).  Cached under param_key(lin.weight) exactly as weight_copy caches `_gf_w8`,
    but made lazily, on the first backward — inference never pays its byte per parameter — and dropped by enable_fp8(module, False)."""
    if getattr(lin, "_gf_w8", None) is None:
        raise GoalForceError("fp8_weight_t: the layer carries no fp8 copy: call enable_fp8 first")
    key = param_key(lin.weight)
    if getattr(lin, "_gf_w8t", None) is None or lin._gf_w8t_key != key:
        lin._gf_w8t, lin._gf_w8t_key = ops.cast_fp8_t(lin.weight.detach()), key
    return lin._gf_w8t


class QuantizedInput:
    """A quantised activation shared by the GEMMs that read the same input: `kind` "fp8" — `data` e4m3 bytes, `scale` fp32 per row;
    "fp4" — MXFP4, `data` packed e2m1 codes, `scale` E8M0 bytes (what ops.layernorm_modulate_mxfp4 / ops.gemm_mxfp4_q4 return).
    `x2`: under lora.set_beside_fp8(True), the bf16 tensor an fp8 input was quantised from, when it was built from one (None otherwise):
    what the LoRA adapters beside an fp8 layer read."""

    def __init__(self, x2=None, data=None, scale=None, kind="fp8"):
        self.kind = kind
        self.x2 = x2 if kind == "fp8" and lora.beside_fp8() else None     # (switch off: the bf16 tensor's lifetime is what it was)
        self.data, self.scale = getattr(ops, _QUANT[kind][2])(x2) if x2 is not None else (data, scale)

    @classmethod
    def layernorm(cls, x2, kind="fp8", **kw):
        """LayerNorm(+affine)(+modulate) of x2 delivered as the input of a `kind` layer (ops.layernorm_modulate_fp8 / _mxfp4)."""
        return cls(None, *getattr(ops, _QUANT[kind][3])(x2, **kw), kind=kind)

    shape = property(lambda self: self.data.shape)
    is_cuda = property(lambda self: self.data.is_cuda)


def linear(x2, lin: nn.Linear, epilogue=ops.EPI_BIAS, resid=None, gate=None, out=None):
    """One nn.Linear on the MFMA GEMM, in the layer's precision(): the bf16 kernel; the reference's fp8_linear contract (enable_fp8;
    VRAM:115-151: per-row dynamic activation scale, unit weight scale, e4m3); ops.gemm_mxfp4 (enable_fp4).  A bf16 x2 is quantised here
    for the layer; a QuantizedInput of the layer's kind reuses one quantisation for several layers, one of another kind is refused.
    out=QuantizedInput (the class): an fp4 layer's result as the next one's input, quantised in the GEMM's epilogue (ops.gemm_mxfp4_q4).
    A bf16 layer with attached LoRA adapters of non-zero strength (lora.attach) runs its GEMM with EPI_BIAS, then per adapter
    ops.gemm for t = x down^T and ops.lora_up, the last one with the caller's epilogue, resid, gate and out.  An enable_fp8 layer with
    live adapters is refused unless lora.set_beside_fp8 is on: then _linear_fp8_lora runs it."""
    kind, given = precision(lin), getattr(x2, "kind", "bf16")
    adapters = lora.live(lin)
    if adapters and kind == "fp8" and lora.beside_fp8():
        return _linear_fp8_lora(x2, lin, adapters, given, epilogue, resid, gate, out)
    if adapters:
        if kind != "bf16":
            raise GoalForceError(f"linear: an attached LoRA adapter ({adapters[0].name!r}) on an enable_{kind} layer is refused: use the "
                                 "merged form (pipe.load_lora) with quantised layers, or lora.detach first")
        if given != "bf16" or out is QuantizedInput:
            raise GoalForceError(f"linear: a QuantizedInput was handed to or asked of a layer with an attached LoRA adapter "
                                 f"({adapters[0].name!r}): attached adapters run on bf16 activations only")
        y = ops.gemm(x2, lin.weight, lin.bias)
        for i, ad in enumerate(adapters):
            ad.on(y.device)
            t = ops.gemm(x2, ad.down)
            if i + 1 < len(adapters):
                ops.lora_up(y, t, ad.up, ad.alpha, out=y)
            else:
                y = ops.lora_up(y, t, ad.up, ad.alpha, epilogue=epilogue, resid=resid, gate=gate, out=y if out is None else out)
        return y
    w = lin.weight if kind == "bf16" else weight_copy(lin, kind)
    if given not in ("bf16", kind):
        raise GoalForceError(f"linear: an {given} QuantizedInput was handed to " + (
            "a bf16 layer" if kind == "bf16" else f"an enable_{kind} layer, which quantises its own bf16 input"))
    if out is QuantizedInput and kind != "fp4":
        raise GoalForceError(f"linear: a QuantizedInput result is what one enable_fp4 layer hands the next; this layer runs in {kind}")
    if kind == "bf16":
        return ops.gemm(x2, w, lin.bias, epilogue=epilogue, resid=resid, gate=gate, out=out)
    q = x2 if given == kind else QuantizedInput(x2, kind=kind)
    if out is QuantizedInput:
        return QuantizedInput(None, *ops.gemm_mxfp4_q4(q.data, q.scale, *w, lin.bias, epilogue=epilogue), kind="fp4")
    gemm, w = (ops.gemm_mxfp4, w) if kind == "fp4" else (ops.gemm_fp8, (w,))
    return gemm(q.data, q.scale, *w, lin.bias, epilogue=epilogue, resid=resid, gate=gate, out=out)


def _linear_fp8_lora(x2, lin, adapters, given, epilogue, resid, gate, out):
    """linear() on an enable_fp8 layer with live adapters under lora.set_beside_fp8: the reference's AutoWrappedLinear.forward
    (VRAM:168-187) — the fp8 product of the quantised x plus every adapter on the bf16 x.  One adapter: ops.gemm_fp8_lora (one launch
    where gf_gemm_fp8_lora runs).  Several: ops.gemm_fp8(EPI_BIAS), then ops.lora_up per adapter in place as the bf16 route chains them,
    the last with the caller's epilogue, resid, gate and out (each adapter's update is rounded into the running bf16 sum, which only
    the materialised y0 can carry)."""
    name = adapters[0].name
    if out is QuantizedInput or given not in ("bf16", "fp8"):
        raise GoalForceError(f"linear: a QuantizedInput was handed to or asked of a layer with an attached LoRA adapter "
                             f"({name!r}): attached adapters run on bf16 activations only")
    q = x2 if given == "fp8" else QuantizedInput(x2)
    xb = q.x2
    if xb is None:
        raise GoalForceError(f"linear: the fp8 QuantizedInput handed to a layer with an attached LoRA adapter ({name!r}) carries no "
                             "bf16 source (QuantizedInput.x2): the adapter reads the unquantised activation — build it from the bf16 tensor")
    w8 = weight_copy(lin, "fp8")
    ts = [ops.gemm(xb, ad.on(q.data.device).down) for ad in adapters]
    if len(adapters) == 1:
        ad = adapters[0]
        return ops.gemm_fp8_lora(q.data, q.scale, w8, lin.bias, ts[0], ad.up, ad.alpha, epilogue=epilogue, resid=resid, gate=gate, out=out)
    y = ops.gemm_fp8(q.data, q.scale, w8, lin.bias)
    for ad, t in zip(adapters[:-1], ts[:-1]):
        ops.lora_up(y, t, ad.up, ad.alpha, out=y)
    ad = adapters[-1]
    return ops.lora_up(y, ts[-1], ad.up, ad.alpha, epilogue=epilogue, resid=resid, gate=gate, out=y if out is None else out)


def enable_fp8(module: nn.Module, enabled=True):
    """BASELINE config 5: every nn.Linear inside the DiT / ControlNet *blocks* runs the fp8_linear contract
    (the reference would set computation_dtype=float8_e4m3fn in enable_vram_management, VRAM:113).  Weights are
    cast once to OCP e4m3 (unit scale) and kept beside the bf16 master copy."""
    for blk in (m for m in module.modules() if isinstance(m, DiTBlock)):
        for lin in (m for m in blk.modules() if isinstance(m, nn.Linear)):
            weight_copy(lin, "fp8", bool(enabled))
            if not enabled and getattr(lin, "_gf_w8t", None) is not None:
                lin._gf_w8t = lin._gf_w8t_key = None      # the backward's transposed copy (fp8_weight_t) goes with it
    return module


FP4_LAYERS = ("ffn", "o")


def fp4_linears(blk: "DiTBlock", layers=FP4_LAYERS):
    """The Linears of a block that the layer names of enable_fp4 stand for."""
    named = {"ffn": (blk.ffn[0], blk.ffn[2]), "o": (blk.self_attn.o, blk.cross_attn.o)}
    return [lin for name in layers for lin in named[name]]


def enable_fp4(module: nn.Module, enabled=True, layers=FP4_LAYERS):
    """MXFP4 linears (include/goalforce.h; the reference has no counterpart, off by default): the named Linears of every DiTBlock
    inside `module` (a block, a WanModel, a ControlNet or a whole pipeline) get an MXFP4 weight copy (ops.quant_mxfp4: e2m1 codes,
    one E8M0 scale per 32 input features) beside the bf16 master, and dit.linear runs them on ops.gemm_mxfp4 with the activation
    quantised the same way per call — the "o" projections by the stand-alone pass, the FFN's two inputs inside the LayerNorm and
    the GELU GEMM's epilogue (DiTBlock.forward; ops.options(fp4_fused=False): the stand-alone pass there too, the same bits).
    "ffn" = ffn[0] and ffn[2], "o" = self_attn.o and cross_attn.o; q / k / v and the
    cross-attention's k / v keep their fused bf16 / fp8 paths and any other name is refused.  An fp4 copy wins over an fp8 copy of
    the same layer (enable_fp8); enabled=False removes the fp4 copies of the named layers and leaves whatever else was there.
    A mechanism: the quality of a trained model under it has not been measured."""
    layers = (layers,) if isinstance(layers, str) else tuple(layers)
    bad = [name for name in layers if name not in FP4_LAYERS]
    if bad:
        raise GoalForceError(f"enable_fp4: unknown layer name {bad[0]!r}: expected a subset of {FP4_LAYERS} "
                             "(q / k / v keep their fused bf16 / fp8 paths)")
    for blk in module.modules():
        if isinstance(blk, DiTBlock):
            for lin in fp4_linears(blk, layers):
                if enabled and lin.weight.shape[1] % 256:
                    raise GoalForceError(f"enable_fp4: a Linear with {lin.weight.shape[1]} input features: gf_gemm_mxfp4 needs a multiple of 256")
                weight_copy(lin, "fp4", bool(enabled))
    return module


def enable_sage_attention(module: nn.Module, enabled=True):
    """The reference's SageAttention branch of flash_attention (DIT:22-26, 50-54: `sageattn(q, k, v)` when the package is installed):
    every SelfAttention inside the DiT / ControlNet blocks of `module` (a WanModel, a ControlNet, a block or a whole pipeline) runs
    ops.sage_attn — smoothed-K int8 QK^T, e4m3 PV, fp32 accumulation — on one GPU (bf16 or fp8 linears) and under head
    parallelism.  Cross-attention stays on the exact kernels; training refuses a switched block (there is no backward).
    enabled=False restores the flash-attention path bit for bit."""
    for blk in module.modules():
        if isinstance(blk, DiTBlock):
            blk.self_attn._gf_sage = bool(enabled)
    return module


def enable_sparse_attention(module: nn.Module, pattern, dense_blocks: int = 0):
    """Block-sparse self-attention (sparse_attention.py; the reference has no counterpart): every SelfAttention inside the DiT /
    ControlNet blocks of `module` (a WanModel, a ControlNet, a block or a whole pipeline) runs ops.flash_attn_sparse on the map
    `pattern(grid)` of the token grid it is called on — a sparse_attention.FrameWindow, or any callable grid -> ops.BlockMap (the
    hook for per-head maps) — or, for a pattern with `from_qk(q, k, num_heads, grid, scale)` (sparse_attention.MassCover), on the
    map built on the device from that attention's own finished q and k.  `dense_blocks` = n keeps the first n blocks of every stack (`.blocks`) on the dense kernel.
    pattern=None restores the dense path bit for bit.  Inference on one GPU only: a switched block refuses training (`keep`),
    sequence parallelism, enable_sage_attention, a caller's own `freqs` (no grid) and key counts below ops.VT_MIN_KV by name instead
    of falling back.  pipe.sparse_dense_steps = n runs the first n sampling steps densely (model_fn_wan_video(sparse_dense=True))."""
    if pattern is not None and not callable(pattern) and not hasattr(pattern, "from_qk"):
        raise GoalForceError(f"enable_sparse_attention: expected a callable grid -> ops.BlockMap (or None), got {type(pattern).__name__}")
    if int(dense_blocks) != dense_blocks or dense_blocks < 0:
        raise GoalForceError(f"enable_sparse_attention: expected dense_blocks >= 0, got {dense_blocks!r}")
    in_stack = set()
    for m in module.modules():
        if isinstance(getattr(m, "blocks", None), nn.ModuleList):
            for i, blk in enumerate(m.blocks):
                if isinstance(blk, DiTBlock):
                    blk.self_attn._gf_sparse = pattern if i >= dense_blocks else None
                    in_stack.add(id(blk))
    for blk in module.modules():
        if isinstance(blk, DiTBlock) and id(blk) not in in_stack:       # a block handed over on its own
            blk.self_attn._gf_sparse = pattern
    return module


def refuse_training(block: "DiTBlock", fp8_frozen: bool = False):
    """What training.DiTBlockFn refuses of a block's switches, before its forward runs.  `fp8_frozen` (training.set_fp8_frozen): an
    enable_fp8 block is accepted when it is frozen — no parameter requires grad, no live adapter: its backward needs dX alone, which
    runs on the fp8 GEMM (training.linear_dx_fp8) — and refused by its first trainable parameter's name otherwise."""
    # the backward recomputes the block on the bf16 kernels: an fp8 / fp4 forward would not be the function differentiated
    for kind in ("fp8", "fp4"):      # (in this order, whichever of the two wins on a layer that carries both)
        if any(precision(m, (kind,)) == kind for m in block.modules()) and not (kind == "fp8" and fp8_frozen):
            raise GoalForceError(f"training through an enable_{kind} block is refused: call enable_{kind}(module, False) first")
    if fp8_frozen and any(precision(m, ("fp8",)) == "fp8" for m in block.modules()):
        # lora.set_beside_fp8: live TRAINABLE adapters are differentiated beside the frozen fp8 layers (their parameters are the only
        # ones that may ask for a gradient); a frozen attached adapter meets the refusal below, as on a bf16 block
        beside = lora.beside_fp8()
        own = {id(p) for _, m in block.named_modules() for ad in lora.live(m) if ad.trainable for p in (ad.down, ad.up)} if beside else ()
        what = next((f"the trainable parameter {n}" for n, p in block.named_parameters() if p.requires_grad and id(p) not in own), None) or next(
            (f"a live LoRA adapter ({n}: {lora.live(m)[0].name!r})" for n, m in block.named_modules() if lora.live(m) and not beside), None)
        if what is not None:
            raise GoalForceError(f"training through an enable_fp8 block is open to frozen blocks only (no weight gradient exists on the fp8 "
                                 f"kernels): this block has {what}: freeze it, or call enable_fp8(module, False) first")
    for name, m in block.named_modules():
        # a frozen attached adapter would be in the forward only; one made by lora.add_trainable is differentiated (training.DiTBlockFn)
        frozen = [ad for ad in lora.live(m) if not ad.trainable]
        if frozen:
            raise GoalForceError(f"training through a block with a live LoRA adapter ({name}: {frozen[0].name!r}) is refused: "
                                 "call lora.detach(module) or lora.set_strength(module, 0) first")
    if getattr(block.self_attn, "_gf_sage", False):
        # no backward exists for the sage backend (nor in the sageattention package): the backward would differentiate another function
        raise GoalForceError("training through a block with enable_sage_attention is refused: call enable_sage_attention(module, False) first")
    if getattr(block.self_attn, "_gf_sparse", None) is not None:
        # there is no sparse backward: the backward recomputes and differentiates the DENSE attention, whatever the keep level
        # (with keep level "none" the forward's own refusal, SelfAttention.attention_backend(keep=...), is never reached)
        raise GoalForceError("training through a block with enable_sparse_attention is refused (there is no sparse backward): "
                             "call enable_sparse_attention(module, None) first")


def q_rotation(rope: RopeTable, head_dim: int, prescale: bool):
    """(q_cos, q_sin, attn_scale) of the self-attention's q: SelfAttention.attend, and training.DiTBlockFn.backward with the
    `prescale` (ops.options(attn_q_prescale)) its forward saw.
    Q leaves its RMSNorm + RoPE kernel already multiplied by c = softmax scale x log2(e) (the rotation table carries the factor:
    RopeTable.scaled), and the attention is called with scale = ln 2, i.e. c = 1 inside — its `Q <- bf16(Q c)` is then exact.
    One rounding of the rotated q instead of two: at peaky logits (std 3) the self-attention kernel is 3.9e-3 from fp64 on a
    twice-rounded Q and at torch SDPA's level (1.8e-3) on this one (tools/fuzz_ops.py, profiles/r06).  Training too (`keep`):
    the backward rebuilds P from q.k and the forward's log-sum-exp, and a forward that rounded Q a second time hands it an lse
    of OTHER scores — rows of P off by 2^-9 of the logit, dQ / dK / dV 1.7e-2 from fp64 at logit std 8 where torch's SDPA
    backward is at 4e-3 (tools/attnbwd_precision.py).  On the pre-scaled q forward and backward see the same scores; the
    backward of the norm + rotation takes the same scaled table (training.DiTBlockFn) and so returns d/d(projection)."""
    if not prescale:
        return rope.cos, rope.sin, None
    return (*rope.scaled(Q_PRESCALE(head_dim)), math.log(2.0))


def _checked_map(block_map) -> ops.BlockMap:
    if not isinstance(block_map, ops.BlockMap):
        raise GoalForceError(f"sparse attention: expected the pattern to return an ops.BlockMap, got {type(block_map).__name__}")
    return block_map


def _sparse_attn_from_qk(pattern, grid, q, k, v, num_heads, vt=None, scale=None):
    """A data-dependent pattern (sparse_attention.MassCover): the map is built from the finished q and k — after norm + RoPE and
    the pre-scaling — with the scale the attention itself gets, on the same stream."""
    block_map = _checked_map(pattern.from_qk(q, k, num_heads, grid, scale))
    return ops.flash_attn_sparse(q, k, v, num_heads, block_map, vt=vt, scale=scale)


def sageattn(q, k, v, tensor_layout="HND", is_causal=False, sm_scale=None, return_lse=False, **kw):
    """Drop-in for `sageattention.sageattn` as the reference calls it (DIT:50-54): q, k, v [B, heads, S, 128] ("HND", the strided
    `rearrange(q, "b s (n d) -> b n s d")` views are fine) or [B, S, heads, 128] ("NHD") bf16 -> the same layout, on
    ops.sage_attn.  sm_scale defaults to 1/sqrt(128).  Causal masks, the log-sum-exp output and head_dim != 128 are refused; the
    package's other keywords (quantisation granularities, accumulator types) are accepted and ignored: the recipe here is fixed."""
    if is_causal:
        raise GoalForceError("sageattn: is_causal=True is not supported (the Wan DiT attention is non-causal)")
    if return_lse:
        raise GoalForceError("sageattn: return_lse=True is not supported")
    if tensor_layout not in ("HND", "NHD"):
        raise GoalForceError(f"sageattn: tensor_layout {tensor_layout!r} (HND or NHD)")
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise GoalForceError("sageattn: q, k, v must be 4-D")
    if q.shape[-1] != 128 or k.shape[-1] != 128 or v.shape[-1] != 128:
        raise GoalForceError(f"sageattn: head_dim {q.shape[-1]} is not supported (the kernel is built for 128)")
    if tensor_layout == "HND":                                   # [B, n, s, d] -> [B, s, n, d]
        q, k, v = (t.transpose(1, 2) for t in (q, k, v))
    B, sq, n, _ = q.shape
    if k.shape[0] != B or v.shape != k.shape or k.shape[2] != n:
        raise GoalForceError("sageattn: q / k / v batch, head or key counts differ")
    out = torch.empty((B, sq, n, 128), dtype=torch.bfloat16, device=q.device)
    for b in range(B):
        # [s, n, 128] -> [s, n*128]: a view when the token rows are contiguous (the reference's `b s (n d)` tensors are), else a copy
        q2, k2, v2 = (t[b].reshape(t.shape[1], n * 128) for t in (q, k, v))
        ops.sage_attn(q2, k2, v2, n, scale=sm_scale, out=out[b].view(sq, n * 128))
    return out.transpose(1, 2) if tensor_layout == "HND" else out


def pad_run(ctx2: torch.Tensor) -> int:
    """First row index n of the run of identical rows that ends the [L, D] tensor (rows n .. L-1 are all equal): L - 1 when the
    last two rows differ.  One comparison kernel and one 8-byte read-back per call.  The run is a property of the embedded context,
    so model_fn_wan_video calls this ONCE per embedded context (ContextCache.pad_n) and hands n to every block."""
    L = ctx2.shape[0]
    if L < 2:
        return max(L - 1, 0)
    differs = (ctx2[1:] != ctx2[:-1]).any(dim=1)                 # differs[i]: row i + 1 != row i
    idx = torch.nonzero(differs)
    return int(idx[-1]) + 1 if idx.numel() else 0


def _tokens2d(x: torch.Tensor) -> torch.Tensor:
    """[1,S,D] or [S,D] -> [S,D] view."""
    if x.dim() == 3:
        if x.shape[0] != 1:
            raise GoalForceError("hot-path modules take batch 1 ([1,S,D]); loop over the batch")
        return x[0]
    return x


# ------------------------------------------------------------------ modules
class RMSNorm(nn.Module):
    """DIT:100-111 (full-width, fp32 math, bf16 weight multiply)."""

    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        y = x.clone()
        ops.rmsnorm_rope(_tokens2d(y), self.weight, None, None, head_dim=8, eps=self.eps)
        return y


class SelfAttention(nn.Module):
    """DIT:124-147."""

    def __init__(self, dim: int, num_heads: int, eps: float = 1e-6):
        super().__init__()
        self.dim, self.num_heads, self.head_dim = dim, num_heads, dim // num_heads
        self.q, self.k, self.v, self.o = (nn.Linear(dim, dim) for _ in range(4))
        self.norm_q, self.norm_k = RMSNorm(dim, eps=eps), RMSNorm(dim, eps=eps)

    def attention_backend(self, rope: RopeTable, tokens: int, sp, keep, dense: bool):
        """The attention this call runs, attn(q, k, v, num_heads, vt=None, scale=None): ops.flash_attn, ops.sage_attn, or — a block
        switched by enable_sparse_attention, unless `dense` — ops.flash_attn_sparse on the pattern's map of rope.grid, built here (a
        static pattern) or per call (from_qk).  Every refusal comes before the first kernel: a switched block never falls back to
        the dense path on its own."""
        sage = getattr(self, "_gf_sage", False)
        if sage and keep is not None:
            raise GoalForceError("training through a block with enable_sage_attention is refused (the sage backend has no backward): "
                                 "call enable_sage_attention(module, False) first")
        pattern = getattr(self, "_gf_sparse", None)
        if pattern is None or dense:
            return ops.sage_attn if sage else ops.flash_attn
        if sage:
            raise GoalForceError("sparse attention with enable_sage_attention is refused (the sage kernel takes no block map): switch one off")
        if keep is not None:
            raise GoalForceError("training through a block with enable_sparse_attention is refused (there is no sparse backward): "
                                 "call enable_sparse_attention(module, None) first")
        if sp is not None:
            raise GoalForceError("sparse attention under sequence parallelism is refused (the head-parallel exchange takes no block map)")
        grid = getattr(rope, "grid", None)
        if grid is None:
            raise GoalForceError("sparse attention needs the token grid: expected a RopeTable built by WanModel.rope_table "
                                 "(RopeTable.from_grid), got rotary phases without one")
        if tokens != grid[0] * grid[1] * grid[2]:
            raise GoalForceError(f"sparse attention: expected {grid[0] * grid[1] * grid[2]} tokens for the grid {grid}, got {tokens}")
        if tokens < ops.VT_MIN_KV:
            raise GoalForceError(f"sparse attention: expected at least {ops.VT_MIN_KV} tokens (ops.VT_MIN_KV, where the self-attention "
                                 f"runs on kernel 3), got {tokens}")
        if hasattr(pattern, "from_qk"):
            return functools.partial(_sparse_attn_from_qk, pattern, grid)
        return functools.partial(ops.flash_attn_sparse, block_map=_checked_map(pattern(grid)).to(rope.cos.device))

    def attend(self, x2: torch.Tensor, rope: RopeTable, sp=None, keep=None, dense=False) -> torch.Tensor:
        """x2 [S,D] -> attention output BEFORE the o projection, [S,D].  With a sequence_parallel.SequenceParallel
        group `sp`, x2 and rope are this rank's token chunk and the heads are exchanged over xGMI (usp_attn_forward,
        diffsynth/distributed/xdit_context_parallel.py:109-131).  `keep` (a dict, training): the attention output and the
        rows' log-sum-exp are stored under "attn" / "lse" so that the backward does not run the attention again; with
        keep["wide"] also the three projections ("qp", "kp" before their norm, "v").  `dense`: a block switched by
        enable_sparse_attention attends densely in this call (pipe.sparse_dense_steps)."""
        attn = self.attention_backend(rope, x2.shape[0], sp, keep, dense)
        fp8 = precision(self.q) == "fp8"         # then: one quantisation for the three projections
        xin = (x2 if isinstance(x2, QuantizedInput) else QuantizedInput(x2)) if fp8 else x2
        q_rot = q_rotation(rope, self.head_dim, ops.option("attn_q_prescale"))
        if keep is not None:
            return self._attend_keep(xin, rope, q_rot, keep, sp)
        if sp is not None:
            return self._attend_head_parallel(xin, rope, q_rot, sp, "sage" if attn is ops.sage_attn else "flash")
        q, k = self._qk(xin, rope, q_rot, None)
        vt = self._vt_from_projection(xin)
        v = linear(xin, self.v) if vt is None else None
        return attn(q, k, v, self.num_heads, vt=vt, scale=q_rot[2])

    def _qk(self, xin, rope, q_rot, keep):
        """The q and k projections, normed and rotated in place (q with the table of q_rotation)."""
        q, k = linear(xin, self.q), linear(xin, self.k)
        if keep is not None and keep.get("wide"):      # training with room to spare: the pre-norm projections stay for the backward
            keep["qp"], keep["kp"] = q, k
            q, k = q.clone(), k.clone()
        ops.rmsnorm_rope(q, self.norm_q.weight, q_rot[0], q_rot[1], self.head_dim, self.norm_q.eps)
        ops.rmsnorm_rope(k, self.norm_k.weight, rope.cos, rope.sin, self.head_dim, self.norm_k.eps)
        return q, k

    def _vt_from_projection(self, xin):
        """Inference on one GPU (attend calls this with neither `sp` nor `keep`): nothing but the attention reads V, so the projection
        writes it straight in the layout the attention kernel wants (gf_linear_vt32: same bits as the plain projection + the
        transpose, one pass over V less; config 5: gf_linear_vt32_fp8).  -> the V^T operand, or None where the plain projection runs."""
        w = self.v.weight
        fp8 = isinstance(xin, QuantizedInput)
        if lora.live(self.v):          # an attached adapter goes through dit.linear: the plain projection runs
            return None
        if not xin.is_cuda or w.shape[0] < 512 or (fp8 and w.shape[1] % 128) or not ops.vt32_ok(xin.shape[0], self.num_heads, self.head_dim):
            return None
        if fp8:
            return ops.linear_vt32_fp8(xin.data, xin.scale, fp8_weight(self.v), self.v.bias)
        return ops.linear_vt32(xin, w, self.v.bias)

    def _attend_head_parallel(self, xin, rope, q_rot, sp, backend):
        """Head-parallel inference: every projection's tokens-for-heads exchange starts as soon as the projection is ready and flies
        under the next one (same kernels on the same values as the plain path: bit-identical, another issue order)."""
        k = linear(xin, self.k)
        ops.rmsnorm_rope(k, self.norm_k.weight, rope.cos, rope.sin, self.head_dim, self.norm_k.eps)
        hk = sp.heads_start(k, self.num_heads)
        hv = sp.heads_start(linear(xin, self.v), self.num_heads)
        q = linear(xin, self.q)
        ops.rmsnorm_rope(q, self.norm_q.weight, q_rot[0], q_rot[1], self.head_dim, self.norm_q.eps)
        hq = sp.heads_start(q, self.num_heads)
        return sp.attention_started(hq, hk, hv, self.num_heads, tuple(q.shape), scale=q_rot[2], backend=backend)

    def _attend_keep(self, xin, rope, q_rot, keep, sp):
        """Training: the plain projections, the attention with its log-sum-exp, and what the backward asked to keep.  (Always the
        flash backend: attention_backend refuses `keep` on every other.)"""
        q, k = self._qk(xin, rope, q_rot, keep)
        v = linear(xin, self.v)
        if sp is not None:
            return sp.attention(q, k, v, self.num_heads, scale=q_rot[2], backend="flash")
        keep["attn"], keep["lse"] = ops.flash_attn_lse(q, k, v, self.num_heads, scale=q_rot[2])
        if keep.get("wide"):
            keep["v"] = v
        return keep["attn"]

    def forward(self, x, freqs):
        x2 = _tokens2d(x)
        a = self.attend(x2, _as_rope(freqs, x.device))
        return linear(a, self.o).view(x.shape)


class CrossAttention(nn.Module):
    """DIT:150-186, has_image_input=False branch (A14B I2V: DIT:703-718)."""

    def __init__(self, dim: int, num_heads: int, eps: float = 1e-6, has_image_input: bool = False):
        super().__init__()
        if has_image_input:
            raise NotImplementedError("has_image_input=True (CLIP image tokens) is outside the Goal-Force path")
        self.dim, self.num_heads, self.head_dim = dim, num_heads, dim // num_heads
        self.q, self.k, self.v, self.o = (nn.Linear(dim, dim) for _ in range(4))
        self.norm_q, self.norm_k = RMSNorm(dim, eps=eps), RMSNorm(dim, eps=eps)
        self.has_image_input = False

    def context_kv(self, ctx2: torch.Tensor, fold: bool = True, pad_n: Optional[int] = None):
        """k = norm_k(Wk ctx), v = Wv ctx — constant per (expert, prompt, block); cacheable over steps.  -> (k, v, m).

        `fold`: the prompter zeroes the text-encoder output past the prompt (wan_prompter.py:99-109), so the padded rows of
        `text_embedding(context)` are all the same vector — and so are their K and V rows (every op here acts row by row).
        softmax over [k_0 .. k_{n-1}, k_pad x m] is evaluated on n + 1 keys with the last one counting m times
        (ops.flash_attn(last_key_mult=m)): the same function of q, 41 keys instead of 512 for a 40-token prompt.  The run is
        DETECTED on the tensor (pad_run), never assumed; a context without such a run is attended in full.  `pad_n` is that
        detection's result when the caller already ran it on this very tensor (model_fn does, once per embedded context, instead
        of one host read-back per block).  `ops.options(fold_pad_keys=False)` switches the folding off (A/B, and the cross-check in
        tests/test_kernels_gpu.py)."""
        m = 1
        if fold and ctx2.is_cuda and ops.option("fold_pad_keys"):
            n = pad_run(ctx2) if pad_n is None else pad_n
            if ctx2.shape[0] - n >= 2 and n + 1 < ops.VT_MIN_KV:      # (the multiplicity form exists for short key sequences only)
                m = ctx2.shape[0] - n
                ctx2 = ctx2[: n + 1]
        cin = QuantizedInput(ctx2) if precision(self.k) == "fp8" else ctx2
        k, v = linear(cin, self.k), linear(cin, self.v)
        ops.rmsnorm_rope(k, self.norm_k.weight, None, None, self.head_dim, self.norm_k.eps)
        return k, v, m

    def attend(self, x2, kv):
        q = linear(x2, self.q)
        ops.rmsnorm_rope(q, self.norm_q.weight, None, None, self.head_dim, self.norm_q.eps)
        return ops.flash_attn(q, kv[0], kv[1], self.num_heads, last_key_mult=kv[2] if len(kv) > 2 else 1)

    # The output projection folded into the cached values: per head the attention output is a mix of the n_keys value
    # rows, so o(a) = sum_h P_h (V_h W_o,h^T) + b — probabilities [S, H*n_pad] times a table U [D, H*n_pad] that is constant per
    # (expert, prompt, block) like K / V: K = H*n_pad instead of D in the projection GEMM (1920 instead of 5120 for a 40-token prompt).
    # n_pad = n_keys + 1 (the last key's rounding residue, ops.cross_probs) rounded up to 16: 48 for a 40-token prompt (41 keys).
    # FOLD_K_MAX: the largest H*n_pad the folded path takes — every shape gf_cross_probs accepts (n_keys <= 63, K <= 2560 at 40 heads)
    # measured faster than attention + D->D GEMM (EXPERIMENTS.md, profiles/r07/crossover.log).
    FOLD_K_MAX = 2560

    def fold_ok(self, kv) -> bool:
        """Does the folded path serve this (inference) forward: pad-folded keys (multiplicity > 1) few enough for one key tile,
        a bf16 o projection (not the fp8_linear contract), no autograd, a GEMM-able K (heads x n_pad a multiple of 64: not the
        2-head test models), ops.options(fold_cross_o) on."""
        if not ops.option("fold_cross_o") or torch.is_grad_enabled() or len(kv) < 3 or kv[2] == 1 or self.head_dim != 128:
            return False
        if precision(self.o) != "bf16" or lora.live(self.o):      # (an attached adapter on o: the unfolded path, through dit.linear)
            return False
        n = kv[0].shape[0]
        k = self.num_heads * self.fold_pad(n)          # the projection GEMM's K: a multiple of 64 (gf_gemm_bf16)
        return n <= ops.CROSS_FOLD_MAX_KEYS and k <= self.FOLD_K_MAX and k % 64 == 0

    @staticmethod
    def fold_pad(n_keys: int) -> int:
        return -(-(n_keys + 1) // 16) * 16

    def fold_table(self, kv):
        """U = V_h W_o,h^T per head, [D, H*n_pad] bf16 (ops.cross_fold_table): model_fn memoises it in ContextCache beside the K / V."""
        return ops.cross_fold_table(kv[1], self.o.weight, self.num_heads, self.fold_pad(kv[0].shape[0]))

    def attend_probs(self, x2, kv):
        """attend() up to the normalised probabilities [S, H*n_pad] (ops.cross_probs) — the A operand of the folded projection."""
        q = linear(x2, self.q)
        ops.rmsnorm_rope(q, self.norm_q.weight, None, None, self.head_dim, self.norm_q.eps)
        return ops.cross_probs(q, kv[0], self.num_heads, self.fold_pad(kv[0].shape[0]), last_key_mult=kv[2])

    def forward(self, x: torch.Tensor, y: torch.Tensor):
        x2 = _tokens2d(x)
        a = self.attend(x2, self.context_kv(_tokens2d(y)))
        return linear(a, self.o).view(x.shape)


class GateModule(nn.Module):
    """DIT:189-194 — `x + gate * residual`.  DiTBlock.forward fuses this into the epilogue of the GEMM that produces `residual`
    (GF_EPI_BIAS_GATE_RESID); the module's own forward is the stand-alone kernel gf_gate_residual with the same bf16 rounding
    order (the product first, then the sum), for callers that use the module directly."""

    def forward(self, x, gate, residual):
        if x.shape != residual.shape:
            raise GoalForceError("GateModule: x and residual must have the same shape")
        d = x.shape[-1]
        g = gate.reshape(-1, d)
        if x.dim() == 3 and g.shape[0] == x.shape[0] and x.shape[0] > 1:        # one gate row per batch element ([B,1,D])
            return torch.stack([ops.gate_residual(x[b], g[b].contiguous(), residual[b]) for b in range(x.shape[0])])
        if g.shape[0] != 1:
            raise GoalForceError("GateModule: gate must be [B or 1, 1, D] (per-token gates are outside the Goal-Force path)")
        return ops.gate_residual(x, g[0].contiguous(), residual)


class DiTBlock(nn.Module):
    """DIT:197-230.  forward(x, context, t_mod, freqs) -> new x; x [1,S,D] bf16, context [1,L,D],
    t_mod [1,6,D], freqs RopeTable (or the reference's complex tensor)."""

    def __init__(self, has_image_input: bool, dim: int, num_heads: int, ffn_dim: int, eps: float = 1e-6):
        super().__init__()
        self.dim, self.num_heads, self.ffn_dim, self.eps = dim, num_heads, ffn_dim, eps
        self.self_attn = SelfAttention(dim, num_heads, eps)
        self.cross_attn = CrossAttention(dim, num_heads, eps, has_image_input=has_image_input)
        self.norm1 = nn.LayerNorm(dim, eps=eps, elementwise_affine=False)
        self.norm2 = nn.LayerNorm(dim, eps=eps, elementwise_affine=False)
        self.norm3 = nn.LayerNorm(dim, eps=eps)
        self.ffn = nn.Sequential(nn.Linear(dim, ffn_dim), nn.GELU(approximate="tanh"), nn.Linear(ffn_dim, dim))
        self.modulation = nn.Parameter(torch.randn(1, 6, dim) / dim ** 0.5)
        self.gate = GateModule()

    _fused_linear = staticmethod(linear)    # the fused fp4 FFN's: a substitute installed as dit.linear sees the layers handed bf16, as ever

    def _normed(self, x2, reader: nn.Linear, out, **kw):
        """LayerNorm(+affine)(+modulate) of x2 as the input of `reader`: for an fp8 layer, and an fp4 one under ops.options(fp4_fused), a
        QuantizedInput (the row never goes to HBM as bf16), else the bf16 buffer `out` (None: a new one) — which is returned."""
        kind = precision(reader)
        if kind == "bf16" or (kind == "fp4" and not ops.option("fp4_fused")):
            return ops.layernorm_modulate(x2, eps=self.eps, out=out, **kw)
        if kind == "fp8" and lora.beside_fp8():
            # an adapter beside the reader — or beside k / v, which read the q projection's input — reads the bf16 row: the two kernels
            # the fused producer stands for (the same codes and scales), the QuantizedInput keeping its source
            sa = self.self_attn
            if any(lora.live(m) for m in ((sa.q, sa.k, sa.v) if reader is sa.q else (reader,))):
                return QuantizedInput(ops.layernorm_modulate(x2, eps=self.eps, **kw))
        return QuantizedInput.layernorm(x2, kind, eps=self.eps, **kw)

    def forward(self, x, context, t_mod, freqs, context_kv=None, out=None, sp=None, keep=None, self_attn_memo=None,
                fold_pad_keys=True, pad_n=None, dense_attn=False):
        """`dense_attn`: SelfAttention.attend's `dense` (a sparse-switched block attends densely in this call).
        `self_attn_memo` (a dict, optional): x + gate_msa * self_attn(modulate(norm1(x))) — the block's first half — does not
        depend on the text context.  The two forwards of a CFG step run this block on IDENTICAL x, t_mod and freqs (block 0 of the
        DiT and of the ControlNet, model_fn_wan_video), so the first stores that half here and the second takes it: same kernels
        on the same inputs, the same bits, one attention and four projections fewer."""
        if t_mod.dim() == 4:
            raise NotImplementedError("per-token t_mod (seperated_timestep) is outside the Goal-Force path")
        x2 = _tokens2d(x)
        rope = _as_rope(freqs, x.device)
        # rows: shift_msa, 1+scale_msa, gate_msa, shift_mlp, 1+scale_mlp, gate_mlp   (DIT:218-219, 64-65)
        mod = ops.modulation(self.modulation, t_mod.contiguous(), onep_mask=0b010010)
        # config 5: every Linear of the block on the fp8_linear contract, all or none (enable_fp8); read from a layer enable_fp4 never takes
        fp8 = precision(self.self_attn.q) == "fp8"
        if self_attn_memo is not None and "x" in self_attn_memo:
            x_new = self_attn_memo.pop("x")
            ev = self_attn_memo.pop("ev", None)
            if ev is not None:      # the other CFG branch may run on another stream (pipeline.cfg_streams): order after its write
                torch.cuda.current_stream(x_new.device).wait_event(ev)
                x_new.record_stream(torch.cuda.current_stream(x_new.device))
            if out is not None:
                x_new = out.copy_(x_new)
            h = None if fp8 else torch.empty_like(x2)
        else:
            h = self._normed(x2, self.self_attn.q, None, scale1p=mod[1], shift=mod[0])                 # DIT:225
            a = self.self_attn.attend(h, rope, sp, keep, dense=dense_attn)
            x_new = out if out is not None else torch.empty_like(x2)
            linear(a, self.self_attn.o, epilogue=ops.EPI_BIAS_GATE_RESID, resid=x2, gate=mod[2], out=x_new)   # DIT:226
            if keep is not None and keep.get("wide"):
                keep["x1"] = x_new.clone()               # (the rest of the block updates x_new in place)
            if self_attn_memo is not None:
                self_attn_memo["x"] = x_new.clone()      # the rest of the block updates x_new in place
                if x_new.is_cuda:
                    self_attn_memo["ev"] = torch.cuda.Event()
                    self_attn_memo["ev"].record(torch.cuda.current_stream(x_new.device))
        buf = None if fp8 else h        # the bf16 buffer of the first LayerNorm serves the other two
        h = self._normed(x_new, self.cross_attn.q, buf, weight=self.norm3.weight, bias=self.norm3.bias)
        if context_kv is None:
            context_kv = self.cross_attn.context_kv(_tokens2d(context), fold=fold_pad_keys and keep is None, pad_n=pad_n)
        ca = self.cross_attn
        if keep is None and not fp8 and ca.fold_ok(context_kv):
            # the o projection folded into the values: P [S, H*n_pad] @ U^T (context_kv[3] is the table model_fn memoised, if any)
            u = context_kv[3] if len(context_kv) > 3 else ca.fold_table(context_kv)
            ops.gemm(ca.attend_probs(h, context_kv), u, ca.o.bias, epilogue=ops.EPI_BIAS_RESID, resid=x_new, out=x_new)  # DIT:227
        else:
            a = ca.attend(h, context_kv)
            linear(a, ca.o, epilogue=ops.EPI_BIAS_RESID, resid=x_new, out=x_new)                        # DIT:227
        if keep is not None and keep.get("wide"):
            keep["x2b"] = x_new.clone()
        # the FFN under enable_fp4 and ops.options(fp4_fused) in three launches: the LayerNorm and the GELU GEMM quantise what they hold
        # in registers, so neither bf16 intermediate ([S, D], [S, F]) exists; the bits of the five-launch route (fp4_fused=False)
        fused = precision(self.ffn[0]) == "fp4" and ops.option("fp4_fused")
        ffn_linear = self._fused_linear if fused else linear
        if fused:       # (enable_fp4 names ffn[0] and ffn[2] together; this route brings both copies up to date before its LayerNorm)
            fp4_weight(self.ffn[0]), fp4_weight(self.ffn[2])
        h = self._normed(x_new, self.ffn[0], buf, scale1p=mod[4], shift=mod[3])                          # DIT:228
        f1 = ffn_linear(h, self.ffn[0], epilogue=ops.EPI_BIAS_GELU_TANH, out=QuantizedInput if fused else None)
        ffn_linear(f1, self.ffn[2], epilogue=ops.EPI_BIAS_GATE_RESID, resid=x_new, gate=mod[5], out=x_new)  # DIT:229
        return x_new.view(x.shape)


LORA_HOSTS = (DiTBlock, SelfAttention, CrossAttention)     # the modules whose Linears all run through linear(): what lora.attach takes


class Head(nn.Module):
    """DIT:253-269."""

    def __init__(self, dim: int, out_dim: int, patch_size: Tuple[int, int, int], eps: float):
        super().__init__()
        self.dim, self.patch_size, self.eps = dim, patch_size, eps
        self.norm = nn.LayerNorm(dim, eps=eps, elementwise_affine=False)
        self.head = nn.Linear(dim, out_dim * math.prod(patch_size))
        self.modulation = nn.Parameter(torch.randn(1, 2, dim) / dim ** 0.5)

    def forward(self, x, t_mod):
        if t_mod.dim() == 3:
            raise NotImplementedError("per-token head modulation is outside the Goal-Force path")
        x2 = _tokens2d(x)
        mod = ops.modulation(self.modulation, t_mod.contiguous(), onep_mask=0b10)   # rows: shift, 1+scale
        h = ops.layernorm_modulate(x2, scale1p=mod[1], shift=mod[0], eps=self.eps)
        y = ops.gemm(h, self.head.weight, self.head.bias)
        return y.view(x.shape[:-1] + (y.shape[-1],))


class WanModel(nn.Module):
    """DIT:272-340.  A14B I2V config: dim 5120, in_dim 36, ffn 13824, out 16, text 4096, freq 256,
    40 heads, 40 layers, has_image_input=False, require_clip_embedding=False (DIT:703-718)."""

    def __init__(self, dim: int, in_dim: int, ffn_dim: int, out_dim: int, text_dim: int, freq_dim: int, eps: float,
                 patch_size: Tuple[int, int, int], num_heads: int, num_layers: int, has_image_input: bool,
                 has_image_pos_emb: bool = False, has_ref_conv: bool = False, add_control_adapter: bool = False,
                 in_dim_control_adapter: int = 24, seperated_timestep: bool = False,
                 require_vae_embedding: bool = True, require_clip_embedding: bool = True,
                 fuse_vae_embedding_in_latents: bool = False):
        super().__init__()
        if has_image_input or has_ref_conv or add_control_adapter or seperated_timestep:
            raise NotImplementedError("only the Wan2.2-I2V-A14B configuration (DIT:703-718) is built")
        if tuple(patch_size) != (1, 2, 2):
            raise NotImplementedError("patch_size must be (1,2,2)")
        self.dim, self.in_dim, self.freq_dim, self.out_dim = dim, in_dim, freq_dim, out_dim
        self.has_image_input = has_image_input
        self.patch_size = tuple(patch_size)
        self.seperated_timestep = seperated_timestep
        self.require_vae_embedding = require_vae_embedding
        self.require_clip_embedding = require_clip_embedding
        self.fuse_vae_embedding_in_latents = fuse_vae_embedding_in_latents
        self.num_heads = num_heads
        self.eps = eps
        self.patch_embedding = nn.Conv3d(in_dim, dim, kernel_size=patch_size, stride=patch_size)
        self.text_embedding = nn.Sequential(nn.Linear(text_dim, dim), nn.GELU(approximate="tanh"), nn.Linear(dim, dim))
        self.time_embedding = nn.Sequential(nn.Linear(freq_dim, dim), nn.SiLU(), nn.Linear(dim, dim))
        self.time_projection = nn.Sequential(nn.SiLU(), nn.Linear(dim, dim * 6))
        self.blocks = nn.ModuleList([DiTBlock(has_image_input, dim, num_heads, ffn_dim, eps) for _ in range(num_layers)])
        self.head = Head(dim, out_dim, patch_size, eps)
        self.freqs = precompute_freqs_cis_3d(dim // num_heads)  # plain CPU tuple, like DIT:328
        self.control_adapter = None
        self._rope_cache = {}
        self._patch_w, self._patch_w_key = None, None  # K-padded [dim, kpad] copy of patch_embedding.weight for the GEMM

    # ---- pieces used by model_fn ---------------------------------------------------------------
    def rope_table(self, f, h, w, device) -> RopeTable:
        key = (f, h, w, str(device))
        if key not in self._rope_cache:
            self._rope_cache[key] = RopeTable.from_grid(self.freqs, f, h, w, device)
        return self._rope_cache[key]

    def rope_table_shard(self, f, h, w, device, sp) -> RopeTable:
        """This rank's slice of the table under sequence parallelism (cached like the full one)."""
        key = (f, h, w, str(device), "sp", sp.rank, sp.size)
        if key not in self._rope_cache:
            self._rope_cache[key] = sp.shard_rope(self.rope_table(f, h, w, device))
        return self._rope_cache[key]

    def time_embed(self, timestep: torch.Tensor):
        """GF:1441-1442 — t [1,D], t_mod [1,6,D]."""
        e = sinusoidal_embedding_1d(self.freq_dim, timestep)
        te = self.time_embedding
        t = ops.gemm(ops.gemm(e, te[0].weight, te[0].bias, epilogue=ops.EPI_BIAS_SILU), te[2].weight, te[2].bias)
        tp = self.time_projection[1]
        t_mod = ops.gemm(ops.act(t, "silu"), tp.weight, tp.bias).unflatten(1, (6, self.dim))
        return t, t_mod

    def embed_text(self, context: torch.Tensor):
        """DIT:309-313 — [1,L,text_dim] -> [1,L,D]."""
        te = self.text_embedding
        c2 = _tokens2d(context)
        y = ops.gemm(ops.gemm(c2, te[0].weight, te[0].bias, epilogue=ops.EPI_BIAS_GELU_TANH), te[2].weight, te[2].bias)
        return y.view(context.shape[:-1] + (self.dim,))

    @staticmethod
    def padded_patch_weight(conv: nn.Conv3d) -> torch.Tensor:
        w = conv.weight
        k = w.shape[1] * 4
        kpad = -(-k // 64) * 64
        wp = torch.zeros((w.shape[0], kpad), dtype=w.dtype, device=w.device)
        wp[:, :k] = w.reshape(w.shape[0], k)
        return wp

    def patchify(self, x: torch.Tensor, control_camera_latents_input: Optional[torch.Tensor] = None, extra=None):
        """DIT:341-349 — Conv3d k=s=(1,2,2) as im2col gather + MFMA GEMM; returns ([1,S,D], (f,h,w)).
        `extra` lets model_fn pass y without materialising cat([latents, y]) (GF:1458)."""
        if control_camera_latents_input is not None:
            raise NotImplementedError("camera control adapter is outside the Goal-Force path")
        if x.shape[0] != 1:
            raise GoalForceError("patchify takes batch 1")
        if self._patch_w is None or self._patch_w_key != param_key(self.patch_embedding.weight):
            self._patch_w = self.padded_patch_weight(self.patch_embedding)
            self._patch_w_key = param_key(self.patch_embedding.weight)
        s0 = x[0].contiguous()
        s1 = None if extra is None else extra[0].contiguous()
        f, hh, ww = s0.shape[1], s0.shape[2] // 2, s0.shape[3] // 2
        cols = ops.patchify_im2col(s0, s1, kpad=self._patch_w.shape[1])
        tok = ops.gemm(cols, self._patch_w, self.patch_embedding.bias)
        return tok.unsqueeze(0), (f, hh, ww)

    def unpatchify(self, x: torch.Tensor, grid_size):
        """DIT:351-356."""
        f, h, w = grid_size
        return ops.unpatchify(_tokens2d(x).contiguous(), self.out_dim, f, h, w).unsqueeze(0)

    def _load_from_state_dict(self, *args, **kwargs):
        self._patch_w = None
        return super()._load_from_state_dict(*args, **kwargs)

    def forward(self, x, timestep, context, clip_feature=None, y=None, **kwargs):
        """DIT:358-... plain forward without ControlNet (model_fn is the Goal-Force entry point)."""
        from .model_fn import model_fn_wan_video
        return model_fn_wan_video(self, latents=x, timestep=timestep, context=context, clip_feature=clip_feature, y=y)

    @staticmethod
    def state_dict_converter():
        raise NotImplementedError("checkpoint key conversion is host-side I/O outside the hot path (SURVEY §2 #9)")


A14B_CONFIG = dict(has_image_input=False, patch_size=(1, 2, 2), in_dim=36, dim=5120, ffn_dim=13824, freq_dim=256,
                   text_dim=4096, out_dim=16, num_heads=40, num_layers=40, eps=1e-6,
                   require_clip_embedding=False)  # DIT:703-718
