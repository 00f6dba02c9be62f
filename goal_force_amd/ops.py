"""Torch-tensor front end of the C ABI (include/goalforce.h).

Every function enqueues exactly the named HIP kernel on torch's current stream; tensors
are only used for device memory + stream plumbing (data_ptr()), never for the arithmetic.
There is no CPU path: tensors must live on a HIP device.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import (EPI_BIAS, EPI_BIAS_GATE_RESID, EPI_BIAS_GELU_TANH, EPI_BIAS_MUL, EPI_BIAS_RESID, EPI_BIAS_SILU,
                   GoalForceError)

__all__ = [
    "modulation", "layernorm_modulate", "rmsnorm_rope", "gate_residual", "gemm", "flash_attn", "flash_attn_sparse", "BlockMap", "block_means", "block_means_coherence", "block_map_scores", "block_map_select", "block_map_from_qk", "patchify_im2col", "unpatchify",
    "cfg_euler_step", "act", "add", "sub", "rel_l1", "force_map", "lora_merge", "lora_up", "lora_grad", "gemm_fp8_lora",
    "EPI_BIAS", "EPI_BIAS_GELU_TANH", "EPI_BIAS_GATE_RESID", "EPI_BIAS_RESID", "EPI_BIAS_SILU", "EPI_BIAS_MUL",
]

_BF16 = torch.bfloat16
_FP8 = torch.float8_e4m3fn

# Optional per-launch timing of the dominant kernel (bench.py's roofline leg): when PROFILE_ATTN is a list,
# flash_attn() brackets every launch with events recorded on the launch stream and appends
# (start, end, q_len, kv_len, heads).  None (default) = no events, no overhead.
PROFILE_ATTN = None
# Same for the GEMM (bench.py's second roofline entry): a list collects (start, end, M, N, K, epilogue) per launch.
PROFILE_GEMM = None
# the same for the VAE convolutions (bench.py's `roofline_vae`): (ev0, ev1, rows, N, C, kt, ks, mode, with_resid) per gf_conv3d_bf16 launch
PROFILE_CONV = None


def _stream(t: torch.Tensor):
    """The HIP stream the launch goes to: torch's current stream of the tensor's device.  The C ABI launches on the
    CURRENT HIP device, so a tensor of another device is refused instead of being launched on the wrong GPU."""
    if t.device.index != torch.cuda.current_device():
        raise GoalForceError(f"tensor lives on cuda:{t.device.index} but the current device is cuda:"
                             f"{torch.cuda.current_device()}: call torch.cuda.set_device (one process per GPU)")
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _req(t: torch.Tensor, name: str, dtype=_BF16):
    if not t.is_cuda:
        raise GoalForceError(f"{name}: tensor must be on the GPU (no CPU fallback exists)")
    if t.dtype != dtype:
        raise GoalForceError(f"{name}: expected dtype {dtype}, got {t.dtype}")


def _rows2d(t: torch.Tensor, name: str):
    """Return (tensor, rows, dim, row_stride) for a tensor whose last dim is contiguous and whose
    leading dims collapse to one row index with a single stride."""
    if t.stride(-1) != 1:
        raise GoalForceError(f"{name}: last dim must be contiguous")
    if t.dim() == 1:
        return t, 1, t.shape[0], t.shape[0]
    v = t.reshape(-1, t.shape[-1]) if t.is_contiguous() else t
    if v.dim() != 2:
        raise GoalForceError(f"{name}: cannot view as [rows, dim] without a copy")
    return v, v.shape[0], v.shape[1], v.stride(0)


def _vec(t, name: str, n: int, dtype=_BF16, required=False):
    """A vector operand (bias, gate, scale ...): `dtype`, n elements, contiguous; None passes unless `required`."""
    if t is None:
        if required:
            raise GoalForceError(f"{name}: required")
        return
    _req(t, name, dtype)
    if t.numel() != n or not t.is_contiguous():
        raise GoalForceError(f"{name}: expected contiguous [{n}]")


def _mat(t: torch.Tensor, name: str, dtype=_BF16):
    """A 2-D operand with contiguous rows (a column slice of a wider tensor is fine; the row stride goes to the kernel)."""
    _req(t, name, dtype)
    if t.dim() != 2 or t.stride(1) != 1:
        raise GoalForceError(f"{name}: expected 2-D with contiguous rows, got {tuple(t.shape)}")


def _weight(w: torch.Tensor, name: str, K: int, dtype=_BF16):
    """A weight matrix [N, K] with contiguous rows -> (N, row stride)."""
    _mat(w, name, dtype)
    if w.shape[1] != K:
        raise GoalForceError(f"{name}: expected [N, {K}] with contiguous rows, got {tuple(w.shape)}")
    return w.shape[0], w.stride(0)


def _out(out, name: str, rows: int, cols: int, device):
    """The [rows, cols] bf16 result: a new tensor, or the caller's `out` (that shape, contiguous rows)."""
    if out is None:
        return torch.empty((rows, cols), dtype=_BF16, device=device)
    _mat(out, name)
    if tuple(out.shape) != (rows, cols):
        raise GoalForceError(f"{name}: expected [{rows}, {cols}], got {tuple(out.shape)}")
    return out


def _flat(op: str, **tensors):
    """The operands of an elementwise kernel: bf16, contiguous, all of one size (None: an optional one left out) -> that size."""
    n = next(iter(tensors.values())).numel()
    for name, t in tensors.items():
        if t is None:
            continue
        _req(t, f"{op}.{name}")
        if not t.is_contiguous() or t.numel() != n:
            raise GoalForceError(f"{op}: {' / '.join(tensors)} must be contiguous and equal-sized")
    return n


def kv_pad(skv: int) -> int:
    """The key length rounded up to the 64-key tile: the row length of the V^T operand."""
    return -(-skv // 64) * 64


class _timed:
    """`with _timed(PROFILE_X, *what):` around a launch: when the list is set (read by the caller, per call), events recorded on
    the launch stream bracket it and (start, end, *what) is appended; None: nothing.  A launch that raised appends nothing."""
    __slots__ = ("prof", "what", "e0")

    def __init__(self, prof, *what):
        self.prof, self.what = prof, what

    def __enter__(self):
        if self.prof is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, exc_type, *exc):
        if self.prof is not None and exc_type is None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.prof.append((self.e0, e1) + self.what)
        return False


def _linear_operands(a, w, scale):
    """The operands of a linear layer -> (a as [M, K] rows, M, K, lda, N, ldw): a [.., K] and w [N, K] bf16, or (`scale` given:
    the fp8_linear contract) a [M, K] and w [N, K] float8_e4m3fn with one fp32 scale per row of a."""
    if scale is None:
        _req(a, "linear: activation")
        av, M, K, lda = _rows2d(a, "linear: activation")
        N, ldw = _weight(w, "linear: weight", K)
    else:
        _mat(a, "fp8 linear: activation", _FP8)
        av, (M, K), lda = a, a.shape, a.stride(0)
        N, ldw = _weight(w, "fp8 linear: weight", K, _FP8)
        _vec(scale, "fp8 linear: row scale", M, torch.float32)
    return av, M, K, lda, N, ldw


def modulation(param, t, onep_mask: int):
    """out[i] = bf16(param[i] + t[i % t_rows]); rows in onep_mask get bf16(1 + .) — gf_modulation.
    param [.., k, dim], t [.., t_rows, dim] -> out [k, dim]."""
    _req(param, "modulation.param")
    _req(t, "modulation.t")
    dim = param.shape[-1]
    k = param.numel() // dim
    t_rows = t.numel() // dim
    if not param.is_contiguous() or not t.is_contiguous() or t.shape[-1] != dim:
        raise GoalForceError("modulation: param/t must be contiguous with equal last dim")
    out = torch.empty((k, dim), dtype=_BF16, device=param.device)
    _lib.check(_lib.load().gf_modulation(_ptr(param), _ptr(t), _ptr(out), k, dim, t_rows, int(onep_mask),
                                         _stream(param)), "gf_modulation")
    return out


LN_QUANT_WIDTHS = (5120, 4096, 1536)   # the wave-per-row widths: the only ones gf_layernorm_modulate_fp8 / _mxfp4 take
LN_FP8_WIDTHS = LN_QUANT_WIDTHS        # (its name from before the MXFP4 producer)


def _layernorm_operands(op, x, weight, bias, scale1p, shift, out=None, widths=None):
    """The checks of the three LayerNorm wrappers, in `op`'s words -> (x as [rows, dim] rows, rows, dim, row stride); None — before
    the vectors are looked at — for a row length outside `widths`, where the caller runs the two-kernel pair and layernorm_modulate
    does the refusing."""
    _req(x, f"{op}.x")
    xv, rows, dim, xs = _rows2d(x, f"{op}.x")
    if widths is not None and dim not in widths:
        return None
    if out is not None:
        _rows2d(out, f"{op}.out")
    for name, vec in (("weight", weight), ("bias", bias), ("scale1p", scale1p), ("shift", shift)):
        _vec(vec, f"{op}.{name}", dim)
    return xv, rows, dim, xs


def layernorm_modulate(x, weight=None, bias=None, scale1p=None, shift=None, eps=1e-6, out=None):
    """LayerNorm(+affine)(+modulate) — gf_layernorm_modulate."""
    xv, rows, dim, xs = _layernorm_operands("layernorm_modulate", x, weight, bias, scale1p, shift, out)
    if out is None:
        out = torch.empty(x.shape, dtype=_BF16, device=x.device)
    ov, _, _, os_ = _rows2d(out, "layernorm_modulate.out")
    _lib.check(_lib.load().gf_layernorm_modulate(_ptr(xv), _ptr(ov), _ptr(weight), _ptr(bias), _ptr(scale1p),
                                                 _ptr(shift), rows, dim, xs, os_, float(eps), _stream(x)),
               "gf_layernorm_modulate")
    return out


def rmsnorm_rope(x, weight, cos=None, sin=None, head_dim=128, eps=1e-6):
    """In-place full-width RMSNorm (+RoPE) — gf_rmsnorm_rope."""
    _req(x, "rmsnorm_rope.x")
    _req(weight, "rmsnorm_rope.weight")
    xv, rows, dim, xs = _rows2d(x, "rmsnorm_rope.x")
    if cos is not None:
        _req(cos, "rmsnorm_rope.cos", torch.float32)
        _req(sin, "rmsnorm_rope.sin", torch.float32)
        if cos.shape != (rows, head_dim // 2) or sin.shape != cos.shape or not cos.is_contiguous() \
                or not sin.is_contiguous():
            raise GoalForceError(f"rmsnorm_rope: cos/sin must be contiguous [{rows}, {head_dim // 2}]")
    _lib.check(_lib.load().gf_rmsnorm_rope(_ptr(xv), _ptr(weight), _ptr(cos), _ptr(sin), rows, dim, head_dim, xs,
                                           float(eps), _stream(x)), "gf_rmsnorm_rope")
    return x


def modulate(x, shift, scale):
    """x * (1 + scale) + shift in the reference's eager bf16 rounding sequence (DIT:64-65) — gf_modulate; shift / scale [dim]."""
    _req(x, "modulate.x")
    xv, rows, dim, xs = _rows2d(x, "modulate.x")
    _vec(shift, "modulate.shift", dim, required=True)
    _vec(scale, "modulate.scale", dim, required=True)
    out = torch.empty(x.shape, dtype=_BF16, device=x.device)
    ov, _, _, os_ = _rows2d(out, "modulate.out")
    _lib.check(_lib.load().gf_modulate(_ptr(xv), _ptr(ov), _ptr(scale), _ptr(shift), rows, dim, xs, os_, _stream(x)), "gf_modulate")
    return out


def gate_residual(x, gate, residual):
    """x + gate * residual in the reference's eager bf16 rounding order (DIT:189-194) — gf_gate_residual; gate [dim]."""
    _req(x, "gate_residual.x")
    _req(residual, "gate_residual.residual")
    xv, rows, dim, xs = _rows2d(x, "gate_residual.x")
    rv, rrows, rdim, rs = _rows2d(residual, "gate_residual.residual")
    if (rrows, rdim) != (rows, dim):
        raise GoalForceError(f"gate_residual: residual must match x [{rows}, {dim}]")
    _vec(gate, "gate_residual.gate", dim, required=True)
    out = torch.empty(x.shape, dtype=_BF16, device=x.device)
    ov, _, _, os_ = _rows2d(out, "gate_residual.out")
    _lib.check(_lib.load().gf_gate_residual(_ptr(xv), _ptr(gate), _ptr(rv), _ptr(ov), rows, dim, xs, rs, os_, _stream(x)),
               "gf_gate_residual")
    return out


def rope_apply(x, cos, sin, head_dim):
    """Rotary embedding alone (DIT:92-97) — gf_rope_apply; x [S, H*head_dim] bf16, cos / sin [S, head_dim/2] fp32 -> new tensor."""
    _req(x, "rope_apply.x")
    xv, rows, dim, xs = _rows2d(x, "rope_apply.x")
    for n, t in (("cos", cos), ("sin", sin)):
        _req(t, f"rope_apply.{n}", torch.float32)
        if tuple(t.shape) != (rows, head_dim // 2) or not t.is_contiguous():
            raise GoalForceError(f"rope_apply.{n}: expected contiguous [{rows}, {head_dim // 2}] fp32")
    out = torch.empty(x.shape, dtype=_BF16, device=x.device)
    ov, _, _, os_ = _rows2d(out, "rope_apply.out")
    _lib.check(_lib.load().gf_rope_apply(_ptr(xv), _ptr(ov), _ptr(cos), _ptr(sin), rows, dim, head_dim, xs, os_, _stream(x)),
               "gf_rope_apply")
    return out


def _gemm_result_operands(op, M, N, out, resid, gate, bias):
    """What a GEMM wrapper takes besides its two factors, checked in `op`'s words (`out` [M, N] is the caller's or new) ->
    (out as rows, ldc, resid as rows or None, ldr)."""
    ov, Mo, No, ldc = _rows2d(out, f"{op}.out")
    if (Mo, No) != (M, N):
        raise GoalForceError(f"{op}.out: expected [{M}, {N}], got [{Mo}, {No}]")
    ldr = 0
    if resid is not None:
        _req(resid, f"{op}.resid")
        resid, Mr, Nr, ldr = _rows2d(resid, f"{op}.resid")
        if (Mr, Nr) != (M, N):
            raise GoalForceError(f"{op}.resid: expected [{M}, {N}], got [{Mr}, {Nr}]")
    _vec(gate, f"{op}.gate", N)
    _vec(bias, f"{op}.bias", N)
    return ov, ldc, resid, ldr


def _gemm(a, w, row_scale, bias, epilogue, resid, gate, out):
    """gemm (row_scale None) and gemm_fp8: one set of checks, then gf_gemm_bf16 / gf_gemm_fp8 (which takes the row scales after ldw)."""
    av, M, K, lda, N, ldw = _linear_operands(a, w, row_scale)
    if out is None:
        out = torch.empty(a.shape[:-1] + (N,), dtype=_BF16, device=a.device)
    ov, ldc, resid, ldr = _gemm_result_operands("gemm[_fp8]", M, N, out, resid, gate, bias)
    lib = _lib.load()
    fn, scale = (lib.gf_gemm_bf16, ()) if row_scale is None else (lib.gf_gemm_fp8, (_ptr(row_scale),))
    with _timed(PROFILE_GEMM, M, N, K, int(epilogue)):
        _lib.check(fn(_ptr(av), lda, _ptr(w), ldw, *scale, _ptr(bias), _ptr(ov), ldc, M, N, K, int(epilogue), _ptr(resid), ldr,
                      _ptr(gate), _stream(a)), fn.__name__)
    return out


def gemm(a, w, bias=None, epilogue=EPI_BIAS, resid=None, gate=None, out=None):
    """out[M,N] = epilogue(a[M,K] @ w[N,K]^T + bias) — gf_gemm_bf16."""
    return _gemm(a, w, None, bias, epilogue, resid, gate, out)


LORA_MAX_RANK = 256


def _lora_scale(op, name, value):
    value = float(value)
    if not math.isfinite(value):
        raise GoalForceError(f"{op}: {name} must be finite, got {value}")
    return value


def lora_merge(w, up, down, alpha=1.0):
    """In place: w[n,k] <- bf16(w + bf16(fp32(alpha) * bf16(sum_j up[n,j] down[j,k]))) — gf_lora_merge (the reference's
    GeneralLoRALoader.load on one weight).  w [n_out, k_in], up [n_out, r], down [r, k_in] bf16 with contiguous rows (row strides go
    to the kernel); 1 <= r <= 256.  The weight's version is bumped, so every copy keyed on it (dit.param_key) is rebuilt; an
    inference tensor has no version: call dit.invalidate_caches() (lora.load does)."""
    for name, t in (("w", w), ("up", up), ("down", down)):
        _mat(t, f"lora_merge.{name}")
        if t.device != w.device:
            raise GoalForceError(f"lora_merge.{name}: lives on {t.device}, w on {w.device}")
    (n_out, k_in), r = w.shape, up.shape[1]
    if up.shape[0] != n_out or tuple(down.shape) != (r, k_in):
        raise GoalForceError(f"lora_merge: w is [{n_out}, {k_in}]: expected up [{n_out}, r] and down [r, {k_in}], got {tuple(up.shape)} "
                             f"and {tuple(down.shape)}")
    if not 1 <= r <= LORA_MAX_RANK:
        raise GoalForceError(f"lora_merge: rank {r}: expected 1 <= r <= {LORA_MAX_RANK}")
    alpha = _lora_scale("lora_merge", "alpha", alpha)
    _lib.check(_lib.load().gf_lora_merge(_ptr(w), w.stride(0), _ptr(up), up.stride(0), _ptr(down), down.stride(0), n_out, k_in, r,
                                         alpha, _stream(w)), "gf_lora_merge")
    # the kernel wrote through the raw pointer: tell torch, as adamw_step does
    if not w.is_inference():
        torch.autograd.graph.increment_version(w)
    return w


def lora_up(y0, t, up, scale, epilogue=EPI_BIAS, resid=None, gate=None, out=None):
    """out[M,N] = epilogue(bf16(y0 + bf16(fp32(scale) * bf16(t[M,R] @ up[N,R]^T))), resid, gate) — gf_lora_up: one attached adapter on
    a layer's output y0 = bf16(acc + bias), t = gemm(x, down_pad); R a multiple of 32, <= 256, up zero beyond the true rank.  `out`
    may be y0 itself (None: a new tensor) or resid."""
    _req(y0, "lora_up.y0")
    yv, M, N, ldy = _rows2d(y0, "lora_up.y0")
    tv, R = _rows_like(t, "lora_up.t", M, t.shape[-1]), t.shape[-1]
    Nu, ld_up = _weight(up, "lora_up.up", R)
    if Nu != N:
        raise GoalForceError(f"lora_up.up: expected [{N}, {R}], got {tuple(up.shape)}")
    if R % 32 or not 32 <= R <= LORA_MAX_RANK:
        raise GoalForceError(f"lora_up: padded rank {R}: expected a multiple of 32 in 32..{LORA_MAX_RANK}")
    scale = _lora_scale("lora_up", "scale", scale)
    if out is None:
        out = torch.empty(y0.shape, dtype=_BF16, device=y0.device)
    ov, ldo, resid, ldr = _gemm_result_operands("lora_up", M, N, out, resid, gate, None)
    _lib.check(_lib.load().gf_lora_up(_ptr(yv), ldy, _ptr(tv[0]), tv[1], _ptr(up), ld_up, _ptr(ov), ldo, M, N, R, scale, int(epilogue),
                                      _ptr(resid), ldr, _ptr(gate), _stream(y0)), "gf_lora_up")
    return out


_LORA_GRAD_WS = {}


def _lora_grad_workspace(nbytes, device):
    """One reusable byte buffer per (device, stream), grown to the largest shape seen — as the block maps' workspace."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _LORA_GRAD_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _LORA_GRAD_WS[key] = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=device)
    return ws


def lora_grad(y, t, scale, transposed=False, out=None):
    """out[C,R] = bf16(fp32(scale) * sum_m y[m,c] t[m,j]) (transposed: out[R,C]) — gf_lora_grad, a trainable adapter's parameter
    gradient: dUp = lora_grad(dy, t, s), dDown = lora_grad(x, dt, s, transposed=True).  y [..., C] and t [..., R] bf16 over the same
    rows (row strides go to the kernel), C % 8 == 0, R a multiple of 32, <= 256.  fp32 sum over the rows, one bf16 rounding; the same
    bits on every call."""
    _req(y, "lora_grad.y")
    yv, M, C, ldy = _rows2d(y, "lora_grad.y")
    R = t.shape[-1]
    tv, ldt = _rows_like(t, "lora_grad.t", M, R)
    if R % 32 or not 32 <= R <= LORA_MAX_RANK:
        raise GoalForceError(f"lora_grad: padded rank {R}: expected a multiple of 32 in 32..{LORA_MAX_RANK}")
    if C % 8:
        raise GoalForceError(f"lora_grad.y: {C} columns: expected a multiple of 8")
    if t.device != y.device:
        raise GoalForceError(f"lora_grad.t: lives on {t.device}, y on {y.device}")
    scale = _lora_scale("lora_grad", "scale", scale)
    rows, cols = (R, C) if transposed else (C, R)
    out = _out(out, "lora_grad.out", rows, cols, y.device)
    lib = _lib.load()
    ws = _lora_grad_workspace(lib.gf_lora_grad_workspace_bytes(M, C, R), y.device)
    _lib.check(lib.gf_lora_grad(_ptr(yv), ldy, _ptr(tv), ldt, _ptr(out), out.stride(0), M, C, R, scale, int(bool(transposed)),
                                _ptr(ws), _stream(y)), "gf_lora_grad")
    return out


VT_MIN_KV = 2048  # key sequences at least this long go through the pre-transposed-V kernel (kernel 3)
# Dispatch overrides.  Every kernel ships, each for the shapes its launcher sends it; the parity tests cross-check two kernels on
# the SAME operands, which needs a way to route a shape to the kernel that would not get it by default.  Nothing here (and nothing
# in the library) reads an environment variable: the defaults are the shipped dispatch and only `options(...)` changes them.
#   library side (gf_set_option): prefer_8wave, a4_stagger, a4_group_m, conv_nb, conv_gather, conv_direct, vae_rms3,
#                attn_fixed_max (0: kernel 3 with the running maximum in ONE launch, instead of the fixed-maximum launch + repair)
#   this module: attn_k3 (False: long key sequences on kernel 2), vt_from_gemm (False: V^T by gf_transpose_v32, not by the V projection),
#                conv_padded (False: the VAE's 192 / 384-channel 3x3x3 convolutions on gf_conv3d_bf16 instead of the padded-layout kernel),
#                fold_pad_keys (False: cross-attention over all 512 context keys instead of the prompt + ONE key of multiplicity, dit.py),
#                attn_q_prescale (False: the self-attention's Q is rotated plainly and scaled inside the attention kernel — a second bf16 rounding),
#                vae_attn_offset (False: the VAE attention's softmax on the bf16-rounded RAW scores — one GEMM instead of two, coarser),
#                fold_cross_o (False: the cross-attention's output projection as attention + D->D GEMM instead of probabilities x the
#                              folded value table, dit.CrossAttention.fold_ok),
#                fp4_fused (False: the FFN of an enable_fp4 block as five launches — LayerNorm, quant_mxfp4, GEMM, quant_mxfp4, GEMM —
#                           instead of three with the quantisation inside the LayerNorm and the GELU GEMM's epilogue; the same bits)
#                fp8_lora_fused (False: gemm_fp8_lora as gemm_fp8 + lora_up, two launches, where gf_gemm_fp8_lora would run; the same bits)
_LIB_DEFAULTS = {"prefer_8wave": 0, "a4_stagger": 2, "a4_group_m": 0, "conv_nb": 0, "conv_gather": 0, "conv_direct": 1, "vae_rms3": 1,
                 "attn_fixed_max": 1}
_OPT = {"attn_k3": True, "vt_from_gemm": True, "conv_padded": True, "fold_pad_keys": True, "attn_q_prescale": True, "vae_attn_offset": True,
        "fold_cross_o": True, "fp4_fused": True, "fp8_lora_fused": True}


def option(name: str) -> bool:
    """The value of a module-side dispatch option (`_OPT`, above) as `ops.options` last set it."""
    return _OPT[name]


def lib_option(name: str) -> int:
    """The value of a library-side dispatch option as the LIBRARY holds it (gf_get_option) — not a Python mirror: a caller that
    used gf_set_option / gf_reset_options directly is seen."""
    import ctypes
    v = ctypes.c_int(0)
    _lib.check(_lib.load().gf_get_option(name.encode(), ctypes.byref(v)), f"gf_get_option({name})")
    return int(v.value)


class options:
    """`with ops.options(prefer_8wave=1): ...` — dispatch overrides for a block, restored afterwards (tests and A/B tools).  The
    restore values are read from the library when the block is entered; an override that fails half-way rolls back the ones
    already applied before the error propagates."""

    def __init__(self, **kv):
        for k in kv:
            if k not in _OPT and k not in _LIB_DEFAULTS:
                raise GoalForceError(f"ops.options: unknown option {k!r}")
        self.kv, self.old = kv, {}

    @staticmethod
    def _apply_one(k, v):
        if k in _OPT:
            _OPT[k] = bool(v)
        else:
            _lib.check(_lib.load().gf_set_option(k.encode(), int(v)), f"gf_set_option({k})")

    def __enter__(self):
        self.old = {}
        try:
            for k, v in self.kv.items():
                old = _OPT[k] if k in _OPT else lib_option(k)
                self._apply_one(k, v)
                self.old[k] = old
        except BaseException:
            self.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, *exc):
        for k, v in reversed(list(self.old.items())):
            self._apply_one(k, v)
        self.old = {}
        return False


_VT_WS = {}


def _vt_workspace(numel, device):
    """One reusable V^T buffer per (device, stream): on one stream the reuse is ordered (every attention launch that reads
    it is enqueued before the next transpose that overwrites it); launches on another stream get their own buffer."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _VT_WS.get(key)
    if ws is None or ws.numel() < numel:
        ws = _VT_WS[key] = torch.empty((numel,), dtype=_BF16, device=device)
    return ws


def _vt_shape(skv, num_heads, head_dim):
    """The shapes of the pre-transposed-V kernels (2 and 3): long key sequences at head_dim 128 whose V^T fits 31-bit indices."""
    return skv >= VT_MIN_KV and head_dim == 128 and num_heads * 128 * kv_pad(skv) < 2 ** 31


def vt32_ok(skv, num_heads, head_dim):
    """True when flash_attn would take the pre-transposed-V kernel 3 for this key length (then linear_vt32 can produce its V^T)."""
    return _vt_shape(skv, num_heads, head_dim) and _OPT["attn_k3"] and _OPT["vt_from_gemm"]


def _linear_vt32(x, w, x_scale, bias):
    """linear_vt32 (x_scale None) and linear_vt32_fp8: gf_linear_vt32 / gf_linear_vt32_fp8 (which takes the row scales after ldx)."""
    xv, skv, K, ldx, N, ldw = _linear_operands(x, w, x_scale)
    _vec(bias, "linear_vt32[_fp8].bias", N)
    vt = _vt_workspace(N * kv_pad(skv), x.device)
    lib = _lib.load()
    fn, scale = (lib.gf_linear_vt32, ()) if x_scale is None else (lib.gf_linear_vt32_fp8, (_ptr(x_scale),))
    _lib.check(fn(_ptr(xv), ldx, *scale, _ptr(w), ldw, _ptr(bias), _ptr(vt), skv, kv_pad(skv), N, K, _stream(x)), fn.__name__)
    return vt


def linear_vt32(x, weight, bias):
    """The V projection of a self-attention, written directly as kernel 3's V^T operand (gf_linear_vt32): returns the V^T
    workspace of this (device, stream) — valid until the next call — for flash_attn(..., vt=...).  Same bits as
    gemm(x, weight, bias) followed by the transpose inside flash_attn."""
    return _linear_vt32(x, weight, None, bias)


def linear_vt32_fp8(x8, x_scale, w8, bias):
    """linear_vt32 on the fp8_linear contract (config 5): x8 [S, K] float8_e4m3fn + its row scales, w8 [N, K] float8_e4m3fn ->
    the V^T workspace (gf_linear_vt32_fp8); same bits as gemm_fp8(x8, x_scale, w8, bias) followed by the transpose."""
    if x_scale is None:
        raise GoalForceError("linear_vt32_fp8.x_scale: required")
    return _linear_vt32(x8, w8, x_scale, bias)


# The flags of the last kernel-3 call on the fixed-maximum path: int32 [heads, query blocks of 256 rows, 8 waves], nonzero where a
# wave's accumulators overflowed and its block was recomputed with the running maximum (tests and tools count repairs with it; a
# fresh tensor per call, so it stays valid).  None after a call that took the exact path (options(attn_fixed_max=0)) or kernel 2.
last_attn_flags = None


def _vt_attn(lib, q, k, v, vt, out, lse, sq, skv, num_heads, head_dim, scale, k3, block_map=None):
    """The attention over a pre-transposed V, shared by flash_attn, flash_attn_lse and flash_attn_sparse: kernel 3 (16x16x32 MFMAs),
    or (k3 False: options(attn_k3=False) for the cross-check tests, a finished q) kernel 2 (32x32x16).  vt None: V^T is made here
    from v.  block_map (a BlockMap, kernel 3 only): gf_flash_attn_fwd_vt32_sparse, which takes the map after lse.  Kernel 3 under
    the library option attn_fixed_max (default on): the _fm entry points — the fixed-maximum launch and its repair launch — with
    a flags workspace of this call's own, which `last_attn_flags` keeps."""
    global last_attn_flags
    tr, fa = (lib.gf_transpose_v32, lib.gf_flash_attn_fwd_vt32) if k3 else (lib.gf_transpose_v, lib.gf_flash_attn_fwd_vt)
    tiles, flags = (), ()
    last_attn_flags = None
    fixed = k3 and lib_option("attn_fixed_max") != 0
    if fixed:
        fa = lib.gf_flash_attn_fwd_vt32_fm
        last_attn_flags = torch.empty((num_heads, -(-sq // 256), 8), dtype=torch.int32, device=q.device)
        flags = (_ptr(last_attn_flags),)
    if block_map is not None:
        fa = lib.gf_flash_attn_fwd_vt32_sparse_fm if fixed else lib.gf_flash_attn_fwd_vt32_sparse
        tiles = (_ptr(block_map.row_ptr), _ptr(block_map.tile_idx), _ptr(block_map.head_map), block_map.n_maps)
    if vt is None:
        vt = _vt_workspace(num_heads * 128 * kv_pad(skv), q.device)
        _lib.check(tr(_ptr(v), v.stride(0), _ptr(vt), skv, kv_pad(skv), num_heads, _stream(q)), "gf_transpose_v")
    _lib.check(fa(_ptr(q), _ptr(k), _ptr(vt), _ptr(out), _ptr(lse), *flags, *tiles, sq, skv, kv_pad(skv), num_heads, head_dim,
                  q.stride(0), k.stride(0), out.stride(0), float(scale), _stream(q)),
               fa.__name__ if tiles or flags else "gf_flash_attn_fwd_vt")


def flash_attn(q, k, v, num_heads, out=None, scale=None, vt=None, last_key_mult=1, finished_q=False):
    """softmax(q k^T / sqrt(d)) v per head; q [Sq, H*128], k/v [Skv, H*128] (row-strided views OK).  `vt` (instead of v): the
    V^T operand linear_vt32 produced for these keys.  `last_key_mult` = m > 1: the last key counts m times (a run of m identical
    trailing keys folded into one: gf_flash_attn_fwd_lastmult; key lengths below the V^T threshold only).
    `finished_q`: q is somebody else's final bf16 tensor (the B3 drop-in dit.flash_attention).  Kernel 3 multiplies Q by
    scale x log2(e) and rounds it to bf16 again — 3.9e-3 / 5.2e-3 from fp64 at logit std 3 / 8 where torch's SDPA is at 1.8e-3 /
    1.7e-3; the package's own modules avoid that by producing q pre-scaled (dit.SelfAttention.attend), a caller with a finished q
    cannot: long key sequences then run on kernel 2, which scales the fp32 scores (2.1e-3 / 1.9e-3; +16 % time at S = 32760,
    profiles/r06/b3_precision.log)."""
    for n, t in (("q", q), ("k", k)) + ((("v", v),) if vt is None else ()):
        _mat(t, f"flash_attn.{n}")
    sq, hd_all = q.shape
    skv = k.shape[0]
    head_dim = hd_all // num_heads
    if k.shape[1] != hd_all or (vt is None and v.shape != k.shape) or head_dim * num_heads != hd_all:
        raise GoalForceError("flash_attn: q/k/v shape mismatch")
    if vt is not None and not vt32_ok(skv, num_heads, head_dim):
        raise GoalForceError("flash_attn: a pre-transposed V is only taken by kernel 3 (key length >= VT_MIN_KV, head_dim 128)")
    if out is None:
        out = torch.empty((sq, hd_all), dtype=_BF16, device=q.device)
    if scale is None:
        scale = 1.0 / math.sqrt(head_dim)
    if last_key_mult != 1 and (vt is not None or skv >= VT_MIN_KV):
        raise GoalForceError("flash_attn: last_key_mult is for short key sequences (the text context), not the V^T path")
    long_keys = _vt_shape(skv, num_heads, head_dim)
    if finished_q and vt is not None:
        raise GoalForceError("flash_attn: finished_q goes to kernel 2, which does not take kernel 3's V^T operand")
    if vt is not None and vt.numel() < num_heads * 128 * kv_pad(skv):
        raise GoalForceError("flash_attn.vt: buffer smaller than heads*128*kv_pad")
    lib = _lib.load()
    with _timed(PROFILE_ATTN, sq, skv, num_heads):
        if long_keys:
            # long key sequences (the DiT self-attention): hand V over pre-transposed — one LDS read per PV MFMA instead of two;
            # the transpose (0.7 % of the attention's time at S=32760) is inside the timed region
            _vt_attn(lib, q, k, v, vt, out, None, sq, skv, num_heads, head_dim, scale, _OPT["attn_k3"] and not finished_q)
        elif last_key_mult != 1:
            _lib.check(lib.gf_flash_attn_fwd_lastmult(_ptr(q), _ptr(k), _ptr(v), _ptr(out), sq, skv, num_heads, head_dim, q.stride(0),
                                                      k.stride(0), v.stride(0), out.stride(0), float(scale), float(last_key_mult),
                                                      _stream(q)), "gf_flash_attn_fwd_lastmult")
        else:
            _lib.check(lib.gf_flash_attn_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), sq, skv, num_heads, head_dim,
                                             q.stride(0), k.stride(0), v.stride(0), out.stride(0), float(scale),
                                             _stream(q)), "gf_flash_attn_fwd")
    return out


# ---- block-sparse self-attention (gf_flash_attn_fwd_vt32_sparse: kernel 3 over a list of key tiles per query block)
SPARSE_QB, SPARSE_KB = 256, 64              # query rows per map row, keys per map column: kernel 3's workgroup and key tile


class BlockMap:
    """Which 64-key tiles every 256-row query block attends to, as the kernel reads it: CSR (`row_ptr` int32
    [n_maps * n_qblocks + 1], `tile_idx` int32 ascending inside a row) and an optional `head_map` int32 [heads] (head h uses map
    head_map[h]; None: every head uses map 0).  Built and validated on the host from a CPU bool array `mask` [n_maps, n_qblocks,
    n_tiles] (a 2-D array is one map), uploaded once (`device`; None keeps it on the host, `to(device)` uploads a copy).
    `q_len` / `kv_len`: the (lowest, highest) sequence lengths the map fits; `density`: selected / all (query block, tile) pairs,
    averaged over the heads when there is a head_map.  The kernel clamps the indices but cannot validate them — this class is
    where a map is checked: every row selects at least 2 tiles (the validated two-tile pipeline).  `from_device` is the one other
    constructor: a map the mass-cover kernels wrote on the device, which the host never reads unless asked."""

    def __init__(self, mask, head_map=None, device=None):
        mask = torch.as_tensor(mask)
        if mask.is_cuda or mask.dtype != torch.bool:
            raise GoalForceError(f"BlockMap.mask: expected a CPU bool array, got {mask.dtype} on {mask.device}")
        if mask.dim() == 2:
            mask = mask[None]
        if mask.dim() != 3 or min(mask.shape) < 1:
            raise GoalForceError(f"BlockMap.mask: expected [n_maps, n_qblocks, n_tiles], got {tuple(mask.shape)}")
        self.n_maps, self.n_qblocks, self.n_tiles = mask.shape
        if self.n_tiles < 2:
            raise GoalForceError(f"BlockMap.mask: expected at least 2 key tiles, got {self.n_tiles}")
        counts = mask.sum(dim=2).reshape(-1)
        if int(counts.min()) < 2:
            m, b = divmod(int(counts.argmin()), self.n_qblocks)
            raise GoalForceError(f"BlockMap.mask: expected at least 2 tiles in every row, got {int(counts.min())} in map {m}, query block {b}")
        if head_map is not None:
            head_map = torch.as_tensor(head_map).to(torch.int64).reshape(-1)
            if head_map.numel() < 1 or int(head_map.min()) < 0 or int(head_map.max()) >= self.n_maps:
                raise GoalForceError(f"BlockMap.head_map: expected map numbers in [0, {self.n_maps}), got {head_map.tolist()}")
            head_map = head_map.to(torch.int32).contiguous()
        row_ptr = torch.zeros(counts.numel() + 1, dtype=torch.int64)
        row_ptr[1:] = counts.cumsum(0)
        self.row_ptr = row_ptr.to(torch.int32)
        self.tile_idx = mask.reshape(-1, self.n_tiles).nonzero()[:, 1].to(torch.int32).contiguous()     # row-major: ascending per row
        self.head_map = head_map
        per_map = counts.reshape(self.n_maps, -1).sum(1).double() / (self.n_qblocks * self.n_tiles)
        self.density = float(per_map.mean() if head_map is None else per_map[head_map.long()].mean())
        self.q_len = ((self.n_qblocks - 1) * SPARSE_QB + 1, self.n_qblocks * SPARSE_QB)
        self.kv_len = ((self.n_tiles - 1) * SPARSE_KB + 1, self.n_tiles * SPARSE_KB)
        if device is not None:
            self._upload(torch.device(device))

    @classmethod
    def from_device(cls, row_ptr, tile_idx, head_map, n_maps, n_qblocks, n_tiles):
        """A map the host never saw (ops.block_map_from_qk / block_map_select wrote it on the device): the CSR tensors are taken as
        they are, on their device, and nothing is read back here — the kernels that write such maps guarantee the contract
        (>= 2 ascending indices < n_tiles per row).  Shapes and dtypes are checked; `counts()` / `mask()` read back on demand, and
        `density` is computed from `counts()` at its first use."""
        try:
            n_maps, n_qblocks, n_tiles = int(n_maps), int(n_qblocks), int(n_tiles)
        except (TypeError, ValueError):
            raise GoalForceError(f"BlockMap.from_device: expected integer n_maps / n_qblocks / n_tiles, got {n_maps!r} / {n_qblocks!r} / {n_tiles!r}") from None
        if n_maps < 1 or n_qblocks < 1 or n_tiles < 2:
            raise GoalForceError(f"BlockMap.from_device: expected n_maps >= 1, n_qblocks >= 1 and n_tiles >= 2, got {n_maps} / {n_qblocks} / {n_tiles}")
        for name, t in (("row_ptr", row_ptr), ("tile_idx", tile_idx)) + ((("head_map", head_map),) if head_map is not None else ()):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
                raise GoalForceError(f"BlockMap.from_device.{name}: expected a contiguous 1-D int32 tensor")
            if t.device != row_ptr.device:
                raise GoalForceError(f"BlockMap.from_device.{name}: expected every tensor on {row_ptr.device}, got {t.device}")
        if row_ptr.numel() != n_maps * n_qblocks + 1:
            raise GoalForceError(f"BlockMap.from_device.row_ptr: expected [{n_maps * n_qblocks + 1}] (n_maps * n_qblocks + 1), got [{row_ptr.numel()}]")
        if tile_idx.numel() < 2 * n_maps * n_qblocks:
            raise GoalForceError(f"BlockMap.from_device.tile_idx: expected room for at least 2 tiles per row ({2 * n_maps * n_qblocks}), "
                                 f"got [{tile_idx.numel()}]")
        self = object.__new__(cls)
        self.n_maps, self.n_qblocks, self.n_tiles = n_maps, n_qblocks, n_tiles
        self.row_ptr, self.tile_idx, self.head_map = row_ptr, tile_idx, head_map
        self.q_len = ((n_qblocks - 1) * SPARSE_QB + 1, n_qblocks * SPARSE_QB)
        self.kv_len = ((n_tiles - 1) * SPARSE_KB + 1, n_tiles * SPARSE_KB)
        return self

    @property
    def density(self):
        """Selected / all (query block, tile) pairs, averaged over the heads when there is a head_map.  A host-built map knows it
        from its mask; a map born on the device (from_device) computes it at the first use, with one read-back of row_ptr."""
        d = self.__dict__.get("_density")
        if d is None:
            per_map = self.counts().sum(1).double() / (self.n_qblocks * self.n_tiles)
            d = self._density = float(per_map.mean() if self.head_map is None else per_map[self.head_map.cpu().long()].mean())
        return d

    @density.setter
    def density(self, value):
        self._density = float(value)

    def forced_bits(self, device):
        """This map (one map for all heads) as the `forced` operand of the mass-cover selection: int32 [n_qblocks, ceil(n_tiles / 32)]
        on `device`, bit t % 32 of word t / 32 set for a selected tile.  Built once per device and kept on the object."""
        if self.n_maps != 1:
            raise GoalForceError(f"BlockMap.forced_bits: expected one map for all heads (the `always` map of a mass cover), got {self.n_maps}")
        device = torch.device(device)
        memo = self.__dict__.setdefault("_forced", {})
        if device not in memo:
            m = self.mask()[0]
            nw = -(-self.n_tiles // 32)
            padded = torch.zeros((self.n_qblocks, nw * 32), dtype=torch.int64)
            padded[:, : self.n_tiles] = m
            words = (padded.reshape(self.n_qblocks, nw, 32) << torch.arange(32)).sum(2)             # < 2^32, as int64
            words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)          # the same 32 bits
            memo[device] = words.contiguous().to(device)
        return memo[device]

    def _upload(self, device):
        self.row_ptr, self.tile_idx = self.row_ptr.to(device), self.tile_idx.to(device)
        if self.head_map is not None:
            self.head_map = self.head_map.to(device)

    @property
    def device(self):
        return self.row_ptr.device

    def to(self, device):
        """The map on `device`: itself when it is there already, else a copy made once per device."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.device:
            return self
        copies = self.__dict__.setdefault("_copies", {})        # uploaded once per device
        if device not in copies:
            other = object.__new__(BlockMap)
            other.__dict__.update({k: v for k, v in self.__dict__.items() if k != "_copies"})
            other._upload(device)
            copies[device] = other
        return copies[device]

    def counts(self):
        """Tiles per row, CPU int64 [n_maps, n_qblocks]."""
        rp = self.row_ptr.cpu().long()
        return (rp[1:] - rp[:-1]).reshape(self.n_maps, self.n_qblocks)

    def mask(self):
        """The bool array the map was built from, rebuilt from the CSR form (CPU)."""
        rows = torch.repeat_interleave(torch.arange(self.n_maps * self.n_qblocks), self.counts().reshape(-1))
        m = torch.zeros((self.n_maps * self.n_qblocks, self.n_tiles), dtype=torch.bool)
        m[rows, self.tile_idx[: rows.numel()].cpu().long()] = True         # (a device-born map's tile_idx is its worst-case buffer)
        return m.reshape(self.n_maps, self.n_qblocks, self.n_tiles)


def flash_attn_sparse(q, k, v, num_heads, block_map, out=None, scale=None, vt=None, lse=False):
    """flash_attn restricted to the key tiles of `block_map` (a BlockMap on q's device): query block b of head h takes its softmax
    over the keys of the tiles the map lists for it and over no others — gf_flash_attn_fwd_vt32_sparse, kernel 3's sparse
    instantiation.  q [Sq, H*128], k / v [Skv, H*128] bf16 (row-strided views OK), Skv >= 128; `vt` (instead of v): the V^T operand
    linear_vt32 / linear_vt32_fp8 wrote for these keys.  lse=True: returns (out, log2-domain log-sum-exp [Sq, H] fp32) over the
    selected keys.  Forward only."""
    for n, t in (("q", q), ("k", k)) + ((("v", v),) if vt is None else ()):
        _mat(t, f"flash_attn_sparse.{n}")
    sq, hd_all = q.shape
    skv = k.shape[0]
    if hd_all != num_heads * 128 or k.shape[1] != hd_all or (vt is None and v.shape != k.shape):
        raise GoalForceError(f"flash_attn_sparse: expected q [Sq, {num_heads}*128] and k / v [Skv, {num_heads}*128], got "
                             f"{tuple(q.shape)} / {tuple(k.shape)}")
    if skv < 2 * SPARSE_KB or sq < 1:
        raise GoalForceError(f"flash_attn_sparse: expected at least 1 query and {2 * SPARSE_KB} keys, got {sq} / {skv}")
    if num_heads * 128 * kv_pad(skv) >= 2 ** 31:
        raise GoalForceError("flash_attn_sparse: expected heads*128*kv_pad below 2^31 elements (the V^T operand's indices)")
    if not isinstance(block_map, BlockMap):
        raise GoalForceError(f"flash_attn_sparse.block_map: expected an ops.BlockMap, got {type(block_map).__name__}")
    if block_map.device != q.device:
        raise GoalForceError(f"flash_attn_sparse.block_map: expected the map on {q.device}, got {block_map.device} (BlockMap.to)")
    if (block_map.n_qblocks, block_map.n_tiles) != (-(-sq // SPARSE_QB), -(-skv // SPARSE_KB)):
        raise GoalForceError(f"flash_attn_sparse.block_map: expected [{-(-sq // SPARSE_QB)} query blocks, {-(-skv // SPARSE_KB)} tiles] for "
                             f"{sq} queries and {skv} keys, got [{block_map.n_qblocks}, {block_map.n_tiles}]")
    if block_map.head_map is not None and block_map.head_map.numel() != num_heads:
        raise GoalForceError(f"flash_attn_sparse.block_map: expected a head_map of [{num_heads}], got [{block_map.head_map.numel()}]")
    if vt is not None and vt.numel() < num_heads * 128 * kv_pad(skv):
        raise GoalForceError("flash_attn_sparse.vt: buffer smaller than heads*128*kv_pad")
    out = _out(out, "flash_attn_sparse.out", sq, hd_all, q.device)
    if scale is None:
        scale = 1.0 / math.sqrt(128)
    lse_t = torch.empty((sq, num_heads), dtype=torch.float32, device=q.device) if lse else None
    # PROFILE_ATTN's key count is what the launch computes: the selected share of the keys (FLOP figures derived from the list count
    # 4 Sq Skv d per head; the dense Skv would overstate a sparse launch by 1 / density).  Evaluated only when profiling is on: the
    # density of a map born on the device (BlockMap.from_device) costs a read-back, which the unprofiled path must not pay
    prof = PROFILE_ATTN
    with _timed(prof, sq, max(1, round(skv * block_map.density)) if prof is not None else skv, num_heads):
        _vt_attn(_lib.load(), q, k, v, vt, out, lse_t, sq, skv, num_heads, 128, scale, True, block_map)
    return (out, lse_t) if lse else out


# ---- mass-cover block maps built on the device from q and k (gf_block_map.hip; the recipe is stated in include/goalforce.h)
BLOCK_MAP_MAX_TILES = 1024
_BLOCK_MAP_WS = {}


def _block_map_rows(t, name, num_heads):
    """A [rows, heads*128] bf16 operand with contiguous rows (a column slice of a wider tensor is fine) -> (rows, row stride)."""
    _mat(t, name)
    if t.shape[1] != num_heads * 128:
        raise GoalForceError(f"{name}: expected [rows, {num_heads}*128] (head_dim 128), got {tuple(t.shape)}")
    if t.shape[0] < 1:
        raise GoalForceError(f"{name}: empty sequence")
    if t.stride(0) % 8 or t.data_ptr() % 16:
        raise GoalForceError(f"{name}: row stride must be a multiple of 8 elements and the data 16-byte aligned")
    return t.shape[0], t.stride(0)


def _block_map_shape(op, sq, skv):
    """(n_qblocks, n_tiles) of a map for sq queries and skv keys; the shapes the selection is not built for are refused by name."""
    if skv < 2 * SPARSE_KB:
        raise GoalForceError(f"{op}: expected at least {2 * SPARSE_KB} keys (two key tiles), got {skv}")
    n_t = -(-skv // SPARSE_KB)
    if n_t > BLOCK_MAP_MAX_TILES:
        raise GoalForceError(f"{op}: expected at most {BLOCK_MAP_MAX_TILES} key tiles ({BLOCK_MAP_MAX_TILES * SPARSE_KB} keys), got {n_t} for {skv} keys")
    return -(-sq // SPARSE_QB), n_t


def _block_map_mass(op, mass):
    try:
        mass = float(mass)
    except (TypeError, ValueError):
        raise GoalForceError(f"{op}.mass: expected a number in (0, 1], got {mass!r}") from None
    if not (0.0 < mass <= 1.0):
        raise GoalForceError(f"{op}.mass: expected 0 < mass <= 1 (the share of the estimated softmax mass to keep), got {mass}")
    return mass


def _block_map_min(op, name, value):
    """A coherence threshold of the gate: None (that side off) or a number in (0, 1]."""
    if value is None:
        return None
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise GoalForceError(f"{op}.{name}: expected a number in (0, 1] (or None), got {value!r}") from None
    if not (0.0 < v <= 1.0):
        raise GoalForceError(f"{op}.{name}: expected 0 < {name} <= 1 (the least coherence a block is predicted for), got {v}")
    return v


def _block_map_coherence(op, name, t, heads, n, device):
    """fp32 contiguous [heads, n] coherences on `device` (ops.block_means_coherence's second result)."""
    _req(t, f"{op}.{name}", torch.float32)
    if t.dim() != 2 or tuple(t.shape) != (heads, n) or not t.is_contiguous():
        raise GoalForceError(f"{op}.{name}: expected contiguous [{heads}, {n}] (heads, blocks), got {tuple(t.shape)}")
    if t.device != device:
        raise GoalForceError(f"{op}.{name}: expected the coherences on {device}, got {t.device}")
    return t


def _block_map_forced(op, always, n_qb, n_t, device):
    if always is None:
        return None
    if not isinstance(always, BlockMap):
        raise GoalForceError(f"{op}.always: expected an ops.BlockMap (or None), got {type(always).__name__}")
    if always.n_maps != 1 or (always.n_qblocks, always.n_tiles) != (n_qb, n_t):
        raise GoalForceError(f"{op}.always: expected one map of [{n_qb} query blocks, {n_t} tiles], got {always.n_maps} of "
                             f"[{always.n_qblocks}, {always.n_tiles}]")
    return always.forced_bits(device)


def _block_map_workspace(nbytes, device):
    """One reusable byte buffer per (device, stream), grown to the largest shape seen — as the sage backend's workspace."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _BLOCK_MAP_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _BLOCK_MAP_WS[key] = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    return ws


def _block_map_out(num_heads, n_qb, n_t, device):
    """The caller-owned CSR buffers of one map: row_ptr, tile_idx at its worst-case capacity, head_map."""
    return (torch.empty((num_heads * n_qb + 1,), dtype=torch.int32, device=device),
            torch.empty((num_heads * n_qb * n_t,), dtype=torch.int32, device=device),
            torch.empty((num_heads,), dtype=torch.int32, device=device))


def block_means(x, num_heads, block):
    """fp32 [heads, ceil(rows / block), 128]: the mean of x [rows, heads*128] bf16 over each run of `block` rows (256: query blocks,
    64: key tiles; a ragged last run divides by its own count) — gf_block_means, a fixed summation order."""
    rows, ldx = _block_map_rows(x, "block_means.x", num_heads)
    if block not in (SPARSE_QB, SPARSE_KB):
        raise GoalForceError(f"block_means.block: expected {SPARSE_QB} (query blocks) or {SPARSE_KB} (key tiles), got {block!r}")
    mean = torch.empty((num_heads, -(-rows // block), 128), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().gf_block_means(_ptr(x), ldx, _ptr(mean), rows, num_heads, block, _stream(x)), "gf_block_means")
    return mean


def block_means_coherence(x, num_heads, block):
    """(mean, coh): block_means(x, num_heads, block) — the same bits — and fp32 [heads, ceil(rows / block)] coherences
    |mean|^2 / mean(|row|^2) of the same runs (gf_block_means_coh, one pass over x): 1 for equal rows, 1/n for orthogonal rows of one
    norm, 0 for rows that cancel, 1 for an all-zero run; NaN for non-finite input (and for finite input whose squares overflow fp32)."""
    rows, ldx = _block_map_rows(x, "block_means_coherence.x", num_heads)
    if block not in (SPARSE_QB, SPARSE_KB):
        raise GoalForceError(f"block_means_coherence.block: expected {SPARSE_QB} (query blocks) or {SPARSE_KB} (key tiles), got {block!r}")
    mean = torch.empty((num_heads, -(-rows // block), 128), dtype=torch.float32, device=x.device)
    coh = torch.empty((num_heads, -(-rows // block)), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().gf_block_means_coh(_ptr(x), ldx, _ptr(mean), _ptr(coh), rows, num_heads, block, _stream(x)), "gf_block_means_coh")
    return mean, coh


def block_map_scores(q_mean, k_mean, q_len, kv_len, scale=None):
    """fp32 [heads, n_qblocks, n_tiles] pooled scores in the log2 domain (gf_block_map_scores): scale x log2(e) x <q_mean, k_mean> +
    log2(keys in the tile), from block_means(q, heads, 256) and block_means(k, heads, 64) of q_len queries and kv_len keys."""
    n_qb, n_t = _block_map_shape("block_map_scores", q_len, kv_len)
    for name, t, n in (("q_mean", q_mean, n_qb), ("k_mean", k_mean, n_t)):
        _req(t, f"block_map_scores.{name}", torch.float32)
        if t.dim() != 3 or t.shape[1:] != (n, 128) or not t.is_contiguous() or t.shape[0] != q_mean.shape[0]:
            raise GoalForceError(f"block_map_scores.{name}: expected contiguous [heads, {n}, 128] for {q_len} queries / {kv_len} keys, "
                                 f"got {tuple(t.shape)}")
    heads = q_mean.shape[0]
    scale = _sage_scale(scale)
    scores = torch.empty((heads, n_qb, n_t), dtype=torch.float32, device=q_mean.device)
    _lib.check(_lib.load().gf_block_map_scores(_ptr(q_mean), _ptr(k_mean), _ptr(scores), q_len, kv_len, heads, scale, _stream(q_mean)),
               "gf_block_map_scores")
    return scores


def block_map_select(scores, mass, always=None, want_kept=False, q_coherence=None, k_coherence=None, q_min=None, k_min=None):
    """The mass-cover selection and its CSR map (gf_block_map_select) from scores fp32 [heads, n_qblocks, n_tiles] (log2 domain): per
    (head, query block) the smallest top set of tiles whose share of sum 2^score reaches `mass`, `always`'s tiles forced in, at
    least 2 tiles, every tile for a row with a non-finite score or mass = 1 -> a BlockMap on the device, one map per head.
    want_kept: (map, fp32 [heads, n_qblocks] estimated kept share).
    The coherence gate (gf_block_map_select_gated; both thresholds None: the ungated entry): with q_min, a query block whose
    q_coherence [heads, n_qblocks] is not >= q_min selects every tile; with k_min, a tile whose k_coherence [heads, n_tiles] is not
    >= k_min is forced for every row of its head.  A threshold and its coherences come together."""
    _req(scores, "block_map_select.scores", torch.float32)
    if scores.dim() != 3 or not scores.is_contiguous() or scores.shape[0] < 1 or scores.shape[1] < 1:
        raise GoalForceError(f"block_map_select.scores: expected contiguous [heads, n_qblocks, n_tiles], got {tuple(scores.shape)}")
    heads, n_qb, n_t = scores.shape
    if not 2 <= n_t <= BLOCK_MAP_MAX_TILES:
        raise GoalForceError(f"block_map_select.scores: expected 2 .. {BLOCK_MAP_MAX_TILES} key tiles, got {n_t}")
    mass = _block_map_mass("block_map_select", mass)
    q_min, k_min = _block_map_min("block_map_select", "q_min", q_min), _block_map_min("block_map_select", "k_min", k_min)
    for name, coh, thr, n in (("q", q_coherence, q_min, n_qb), ("k", k_coherence, k_min, n_t)):
        if (coh is None) != (thr is None):
            raise GoalForceError(f"block_map_select.{name}_coherence: expected {name}_coherence and {name}_min together (or neither), got "
                                 f"{name}_coherence={'None' if coh is None else 'a tensor'}, {name}_min={thr}")
        if coh is not None:
            _block_map_coherence("block_map_select", f"{name}_coherence", coh, heads, n, scores.device)
    forced = _block_map_forced("block_map_select", always, n_qb, n_t, scores.device)
    lib = _lib.load()
    ws = _block_map_workspace(int(lib.gf_block_map_select_workspace_bytes(n_qb, n_t, heads)), scores.device)
    row_ptr, tile_idx, head_map = _block_map_out(heads, n_qb, n_t, scores.device)
    kept = torch.empty((heads, n_qb), dtype=torch.float32, device=scores.device) if want_kept else None
    if q_min is None and k_min is None:
        _lib.check(lib.gf_block_map_select(_ptr(scores), _ptr(forced), _ptr(row_ptr), _ptr(tile_idx), _ptr(head_map), _ptr(kept), _ptr(ws),
                                           n_qb, n_t, heads, mass, _stream(scores)), "gf_block_map_select")
    else:
        # a side that is off goes as a null pointer; its threshold is then not read (1.0 passes the entry's range check)
        _lib.check(lib.gf_block_map_select_gated(_ptr(scores), _ptr(forced), _ptr(q_coherence), _ptr(k_coherence), _ptr(row_ptr),
                                                 _ptr(tile_idx), _ptr(head_map), _ptr(kept), _ptr(ws), n_qb, n_t, heads, mass,
                                                 1.0 if q_min is None else q_min, 1.0 if k_min is None else k_min, _stream(scores)),
                   "gf_block_map_select_gated")
    bm = BlockMap.from_device(row_ptr, tile_idx, head_map, heads, n_qb, n_t)
    return (bm, kept) if want_kept else bm


def block_map_from_qk(q, k, num_heads, mass, always=None, scale=None, workspace=None, want_scores=False, q_min=None, k_min=None,
                      want_coherence=False):
    """The mass-cover map of one self-attention, built on the device from its own operands (gf_block_map_from_qk: pooled means,
    pooled scores, selection, CSR — on the current stream, no host read): q [Sq, H*128], k [Skv, H*128] bf16 (row-strided views
    OK), `scale` the softmax scale the attention will use (default 1/sqrt(128)), `mass` the share of the ESTIMATED softmax mass
    every (head, query block) keeps, `always` an ops.BlockMap of one map whose tiles are kept whatever their score.  -> the
    ops.BlockMap for flash_attn_sparse (one map per head); want_scores: (map, scores fp32 [H, n_qblocks, n_tiles], estimated kept
    share fp32 [H, n_qblocks]).  `workspace`: a uint8 tensor of at least gf_block_map_workspace_bytes bytes (default: the one kept
    per device and stream).
    q_min / k_min (numbers in (0, 1], or None): the coherence gate — gf_block_map_from_qk_gated, whose workspace is
    gf_block_map_gated_workspace_bytes: a query block whose rows are less coherent than q_min (|mean|^2 / mean |row|^2) keeps every
    tile, a key tile less coherent than k_min is kept by every row of its head.  want_coherence: the result is followed by
    (q_coherence fp32 [H, n_qblocks], k_coherence fp32 [H, n_tiles]).  Both thresholds None and no want_coherence: the ungated entry."""
    sq, ldq = _block_map_rows(q, "block_map_from_qk.q", num_heads)
    skv, ldk = _block_map_rows(k, "block_map_from_qk.k", num_heads)
    if k.device != q.device:
        raise GoalForceError(f"block_map_from_qk: expected q and k on one device, got {q.device} / {k.device}")
    n_qb, n_t = _block_map_shape("block_map_from_qk", sq, skv)
    mass = _block_map_mass("block_map_from_qk", mass)
    q_min, k_min = _block_map_min("block_map_from_qk", "q_min", q_min), _block_map_min("block_map_from_qk", "k_min", k_min)
    gated = q_min is not None or k_min is not None or bool(want_coherence)
    scale = _sage_scale(scale)
    forced = _block_map_forced("block_map_from_qk", always, n_qb, n_t, q.device)
    lib = _lib.load()
    nbytes = int((lib.gf_block_map_gated_workspace_bytes if gated else lib.gf_block_map_workspace_bytes)(sq, skv, num_heads))
    if workspace is None:
        workspace = _block_map_workspace(nbytes, q.device)
    else:
        _req(workspace, "block_map_from_qk.workspace", torch.uint8)
        if workspace.numel() < nbytes or not workspace.is_contiguous() or workspace.data_ptr() % 256 or workspace.device != q.device:
            raise GoalForceError(f"block_map_from_qk.workspace: expected a contiguous, 256-byte aligned uint8 buffer of at least {nbytes} "
                                 f"bytes on {q.device}")
    row_ptr, tile_idx, head_map = _block_map_out(num_heads, n_qb, n_t, q.device)
    scores = torch.empty((num_heads, n_qb, n_t), dtype=torch.float32, device=q.device) if want_scores else None
    kept = torch.empty((num_heads, n_qb), dtype=torch.float32, device=q.device) if want_scores else None
    q_coh = torch.empty((num_heads, n_qb), dtype=torch.float32, device=q.device) if want_coherence else None
    k_coh = torch.empty((num_heads, n_t), dtype=torch.float32, device=q.device) if want_coherence else None
    if gated:
        # a threshold of 0 switches that side of the gate off in this entry
        _lib.check(lib.gf_block_map_from_qk_gated(_ptr(q), ldq, _ptr(k), ldk, _ptr(forced), _ptr(row_ptr), _ptr(tile_idx), _ptr(head_map),
                                                  _ptr(scores), _ptr(kept), _ptr(q_coh), _ptr(k_coh), _ptr(workspace), sq, skv, num_heads,
                                                  scale, mass, 0.0 if q_min is None else q_min, 0.0 if k_min is None else k_min,
                                                  _stream(q)), "gf_block_map_from_qk_gated")
    else:
        _lib.check(lib.gf_block_map_from_qk(_ptr(q), ldq, _ptr(k), ldk, _ptr(forced), _ptr(row_ptr), _ptr(tile_idx), _ptr(head_map),
                                            _ptr(scores), _ptr(kept), _ptr(workspace), sq, skv, num_heads, scale, mass, _stream(q)),
                   "gf_block_map_from_qk")
    bm = BlockMap.from_device(row_ptr, tile_idx, head_map, num_heads, n_qb, n_t)
    out = (bm, scores, kept) if want_scores else (bm,)
    if want_coherence:
        out = out + (q_coh, k_coh)
    return out if len(out) > 1 else bm


# ---- SageAttention backend (gf_sage_attention.hip; the recipe is stated in include/goalforce.h)
SAGE_T, SAGE_TAU, SAGE_E = 128, 0, 8        # the kernel's key tile, lazy-rescale threshold and exponent offset
SAGE_QBLK, SAGE_KBLK = 32, 64               # query rows per Q scale, keys per K scale
_SAGE_WS = {}
_SAGE_SCRATCH_PER_HEAD = 64 * 128 * 8


def _sage_rows(t, name, num_heads):
    """A [rows, >= heads*128] bf16 operand with contiguous rows (a column slice of a wider tensor is fine) -> (rows, row stride)."""
    _mat(t, name)
    if t.shape[1] != num_heads * 128:
        raise GoalForceError(f"{name}: {t.shape[1]} columns for {num_heads} heads: the sage backend is built for head_dim 128")
    if t.shape[0] < 1:
        raise GoalForceError(f"{name}: empty sequence")
    if t.stride(0) % 8 or t.data_ptr() % 16:
        raise GoalForceError(f"{name}: row stride must be a multiple of 8 elements and the data 16-byte aligned")
    return t.shape[0], t.stride(0)


def _sage_scale(scale):
    """The softmax scale: 1/sqrt(128) by default; positive and finite (the kernel takes the row maximum on the int32 dots)."""
    scale = 1.0 / math.sqrt(128) if scale is None else float(scale)
    if not (0.0 < scale < math.inf):
        raise GoalForceError(f"sage attention: the softmax scale must be positive and finite, got {scale}")
    return scale


def _sage_scratch(num_heads, device):
    return torch.empty((num_heads * _SAGE_SCRATCH_PER_HEAD,), dtype=torch.uint8, device=device)


def sage_k_mean(k, num_heads):
    """mu [heads, 128] fp32: the per-channel mean of k over its keys (gf_sage_k_mean; fp64 sums, one rounding)."""
    skv, ldk = _sage_rows(k, "sage_k_mean.k", num_heads)
    mu = torch.empty((num_heads, 128), dtype=torch.float32, device=k.device)
    _lib.check(_lib.load().gf_sage_k_mean(_ptr(k), ldk, _ptr(mu), _ptr(_sage_scratch(num_heads, k.device)), skv, num_heads, _stream(k)),
               "gf_sage_k_mean")
    return mu


def sage_quant_q(q, num_heads):
    """(q8 [Sq, heads*128] int8, q_scale [heads, ceil(Sq/32)] fp32): one scale per (head, 32 rows) (gf_sage_quant_q)."""
    sq, ldq = _sage_rows(q, "sage_quant_q.q", num_heads)
    q8 = torch.empty((sq, num_heads * 128), dtype=torch.int8, device=q.device)
    sc = torch.empty((num_heads, -(-sq // SAGE_QBLK)), dtype=torch.float32, device=q.device)
    _lib.check(_lib.load().gf_sage_quant_q(_ptr(q), ldq, _ptr(q8), _ptr(sc), sq, num_heads, _stream(q)), "gf_sage_quant_q")
    return q8, sc


def sage_quant_k(k, num_heads, mu=None):
    """(k8 [kv_pad8, heads*128] int8, k_scale [heads, kv_pad8/64] fp32, mu) of the smoothed k - mu (gf_sage_quant_k); kv_pad8 = keys
    rounded up to 128, rows past the keys zero.  mu defaults to sage_k_mean(k)."""
    skv, ldk = _sage_rows(k, "sage_quant_k.k", num_heads)
    if mu is None:
        mu = sage_k_mean(k, num_heads)
    _vec(mu, "sage_quant_k.mu", num_heads * 128, torch.float32)
    kv_pad8 = -(-skv // SAGE_T) * SAGE_T
    k8 = torch.empty((kv_pad8, num_heads * 128), dtype=torch.int8, device=k.device)
    sc = torch.empty((num_heads, kv_pad8 // SAGE_KBLK), dtype=torch.float32, device=k.device)
    _lib.check(_lib.load().gf_sage_quant_k(_ptr(k), ldk, _ptr(mu), _ptr(k8), _ptr(sc), skv, num_heads, _stream(k)), "gf_sage_quant_k")
    return k8, sc, mu


def sage_quant_vt(v, num_heads, vt=None, kv_len=None):
    """(vt8 [heads*128, kv_pad8] e4m3 as uint8, v_scale [heads, 128] fp32) (gf_sage_quant_vt): V^T in the PV MFMA's key order, one
    scale per channel.  From v [S, heads*128] bf16, or (v None) from the bf16 V^T `vt` that linear_vt32 / linear_vt32_fp8 wrote for
    kv_len keys."""
    if vt is None:
        skv, ldv = _sage_rows(v, "sage_quant_vt.v", num_heads)
        src, vt_in = v, 0
    else:
        _req(vt, "sage_quant_vt.vt")
        if kv_len is None or kv_len < 1:
            raise GoalForceError("sage_quant_vt: a V^T input needs kv_len")
        skv, ldv, src, vt_in = kv_len, kv_pad(kv_len), vt, 1
        if vt.numel() < num_heads * 128 * ldv:
            raise GoalForceError("sage_quant_vt.vt: buffer smaller than heads*128*kv_pad")
    kv_pad8 = -(-skv // SAGE_T) * SAGE_T
    vt8 = torch.empty((num_heads * 128, kv_pad8), dtype=torch.uint8, device=src.device)
    sc = torch.empty((num_heads, 128), dtype=torch.float32, device=src.device)
    _lib.check(_lib.load().gf_sage_quant_vt(_ptr(src), ldv, vt_in, _ptr(vt8), _ptr(sc), _ptr(_sage_scratch(num_heads, src.device)), skv,
                                            num_heads, _stream(src)), "gf_sage_quant_vt")
    return vt8, sc


def sage_attn_quantized(q8, q_scale, k8, k_scale, vt8, v_scale, kv_len, num_heads, scale=None, out=None):
    """The attention kernel alone (gf_sage_attn_fwd) on the operands of sage_quant_q / _k / _vt."""
    sq = q8.shape[0]
    scale = _sage_scale(scale)
    if out is None:
        out = torch.empty((sq, num_heads * 128), dtype=_BF16, device=q8.device)
    _lib.check(_lib.load().gf_sage_attn_fwd(_ptr(q8), _ptr(q_scale), _ptr(k8), _ptr(k_scale), _ptr(vt8), _ptr(v_scale), _ptr(out),
                                            out.stride(0), sq, kv_len, num_heads, scale, _stream(q8)), "gf_sage_attn_fwd")
    return out


def sage_attn(q, k, v, num_heads, scale=None, vt=None, out=None):
    """SageAttention-style softmax(q k^T * scale) v per head (gf_sage_attn: K smoothing, int8 QK^T, e4m3 PV, fp32 accumulation);
    q [Sq, H*128], k / v [Skv, H*128] bf16 with contiguous rows (column slices OK).  `vt` (instead of v): the bf16 V^T that
    linear_vt32 / linear_vt32_fp8 wrote for these keys.  scale defaults to 1/sqrt(128).  Workspace: one reusable buffer per
    (device, stream), as the V^T workspace."""
    scale = _sage_scale(scale)
    sq, ldq = _sage_rows(q, "sage_attn.q", num_heads)
    skv, ldk = _sage_rows(k, "sage_attn.k", num_heads)
    if vt is None:
        sv, ldv = _sage_rows(v, "sage_attn.v", num_heads)
        if sv != skv:
            raise GoalForceError(f"sage_attn: k has {skv} keys, v {sv}")
        src, vt_in = v, 0
    else:
        _req(vt, "sage_attn.vt")
        ldv, src, vt_in = kv_pad(skv), vt, 1
        if vt.numel() < num_heads * 128 * ldv:
            raise GoalForceError("sage_attn.vt: buffer smaller than heads*128*kv_pad")
    out = _out(out, "sage_attn.out", sq, num_heads * 128, q.device)
    if out.stride(0) % 8:
        raise GoalForceError("sage_attn.out: row stride must be a multiple of 8 elements")
    lib = _lib.load()
    nbytes = int(lib.gf_sage_workspace_bytes(sq, skv, num_heads))
    key = (q.device.index, torch.cuda.current_stream(q.device).cuda_stream)
    ws = _SAGE_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _SAGE_WS[key] = torch.empty((nbytes,), dtype=torch.uint8, device=q.device)
    with _timed(PROFILE_ATTN, sq, skv, num_heads):
        _lib.check(lib.gf_sage_attn(_ptr(q), ldq, _ptr(k), ldk, _ptr(src), ldv, vt_in, _ptr(out), out.stride(0), sq, skv, num_heads,
                                    scale, _ptr(ws), _stream(q)), "gf_sage_attn")
    return out


CROSS_FOLD_MAX_KEYS = 63   # gf_cross_probs holds a row's keys and the last key's residue column in one 64-key tile


def cross_probs(q, k, num_heads, n_pad, last_key_mult=1, scale=None, out=None):
    """The normalised probabilities of softmax(q k^T / sqrt(d)) per head instead of the attention output (gf_cross_probs):
    q [Sq, H*128], k [n_keys <= 63, H*128] (row-strided views OK) -> [Sq, H*n_pad] bf16 (n_pad > n_keys), column h*n_pad + j = key j
    of head h; column n_keys: the last key's rounding residue bf16(w - bf16(w)); zero after it.  `last_key_mult` as in flash_attn.  With U = cross_fold_table(v, w_o, H, n_pad), P @ U^T = flash_attn(q, k, v) @ w_o^T."""
    _mat(q, "cross_probs.q")
    _mat(k, "cross_probs.k")
    sq, hd_all = q.shape
    n_keys = k.shape[0]
    head_dim = hd_all // num_heads
    if k.shape[1] != hd_all or head_dim * num_heads != hd_all:
        raise GoalForceError("cross_probs: q/k shape mismatch")
    out = _out(out, "cross_probs.out", sq, num_heads * n_pad, q.device)
    if scale is None:
        scale = 1.0 / math.sqrt(head_dim)
    _lib.check(_lib.load().gf_cross_probs(_ptr(q), _ptr(k), _ptr(out), sq, n_keys, n_pad, num_heads, head_dim, q.stride(0), k.stride(0),
                                          out.stride(0), float(scale), float(last_key_mult), _stream(q)), "gf_cross_probs")
    return out


def cross_fold_table(v, w_o, num_heads, n_pad):
    """The value table of cross_probs (gf_cross_fold_table): U [N, H*n_pad] bf16, U[n, h*n_pad + j] = sum_d v[j, h*128+d] w_o[n, h*128+d]
    (fp32 accumulation, one rounding) for j < n_keys, column n_keys = column n_keys - 1 (the partner of cross_probs' residue column),
    zero after it — the [N, K] weight layout gemm takes."""
    _mat(v, "cross_fold_table.v")
    n_keys, hd_all = v.shape
    N, ldw = _weight(w_o, "cross_fold_table.w_o", hd_all)
    if hd_all % num_heads:
        raise GoalForceError(f"cross_fold_table: {hd_all} columns do not divide into {num_heads} heads")
    u = torch.empty((N, num_heads * n_pad), dtype=_BF16, device=v.device)
    _lib.check(_lib.load().gf_cross_fold_table(_ptr(v), _ptr(w_o), _ptr(u), n_keys, n_pad, num_heads, hd_all // num_heads, N, v.stride(0),
                                               ldw, u.stride(0), _stream(v)), "gf_cross_fold_table")
    return u


def flash_attn_lse(q, k, v, num_heads, scale=None):
    """flash_attn that also returns the log2-domain log-sum-exp [Sq, H] fp32 (what flash_attn_bwd rebuilds P from)."""
    for n, t in (("q", q), ("k", k), ("v", v)):
        _mat(t, f"flash_attn_lse.{n}")
    sq, hd_all = q.shape
    skv = k.shape[0]
    head_dim = hd_all // num_heads
    if k.shape[1] != hd_all or v.shape != k.shape or head_dim * num_heads != hd_all:
        raise GoalForceError("flash_attn_lse: q/k/v shape mismatch")
    if scale is None:
        scale = 1.0 / math.sqrt(head_dim)
    out = torch.empty((sq, hd_all), dtype=_BF16, device=q.device)
    lse = torch.empty((sq, num_heads), dtype=torch.float32, device=q.device)
    lib = _lib.load()
    if _vt_shape(skv, num_heads, head_dim):   # as flash_attn: pre-transposed V, same bits
        _vt_attn(lib, q, k, v, None, out, lse, sq, skv, num_heads, head_dim, scale, _OPT["attn_k3"])
        return out, lse
    _lib.check(lib.gf_flash_attn_fwd_lse(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), sq, skv, num_heads, head_dim,
                                         q.stride(0), k.stride(0), v.stride(0), out.stride(0), float(scale),
                                         _stream(q)), "gf_flash_attn_fwd_lse")
    return out, lse


def flash_attn_bwd(q, k, v, o, dout, lse, num_heads, scale=None, need_dkv=True):
    """Gradients of flash_attn: (dq [Sq, H*128], dk, dv [Skv, H*128]) bf16; need_dkv=False: (dq, None, None) — the dK/dV kernel is
    not launched (a frozen block's cross-attention: nobody reads the gradients of the text context)."""
    for n, t in (("q", q), ("k", k), ("v", v), ("o", o), ("dout", dout)):
        _mat(t, f"flash_attn_bwd.{n}")
    sq, hd_all = q.shape
    skv = k.shape[0]
    head_dim = hd_all // num_heads
    if scale is None:
        scale = 1.0 / math.sqrt(head_dim)
    if lse.dtype != torch.float32 or tuple(lse.shape) != (sq, num_heads) or not lse.is_contiguous():
        raise GoalForceError("flash_attn_bwd.lse: expected contiguous fp32 [Sq, heads]")
    dq = torch.empty_like(q, memory_format=torch.contiguous_format)
    dk = torch.empty((skv, hd_all), dtype=_BF16, device=q.device) if need_dkv else None
    dv = torch.empty((skv, hd_all), dtype=_BF16, device=q.device) if need_dkv else None
    lib = _lib.load()
    # rowsum(dout * o) and the transposed copies of k, q, dout the kernels stream; scratch, sized by the library
    ws = torch.empty((int(lib.gf_flash_attn_bwd_workspace_bytes(sq, skv, num_heads)),), dtype=torch.uint8, device=q.device)
    _lib.check(lib.gf_flash_attn_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(dout), _ptr(lse), _ptr(ws), _ptr(dq),
                                             _ptr(dk) if need_dkv else None, _ptr(dv) if need_dkv else None, sq, skv, num_heads, head_dim,
                                             q.stride(0), k.stride(0), v.stride(0), o.stride(0), dout.stride(0), dq.stride(0),
                                             dk.stride(0) if need_dkv else hd_all, dv.stride(0) if need_dkv else hd_all, float(scale),
                                             _stream(q)), "gf_flash_attn_bwd")
    return dq, dk, dv


def patchify_im2col(src0, src1=None, kpad=None):
    """[c,F,H,W] (+[c1,F,H,W]) -> [F*(H/2)*(W/2), kpad] token-major patches (Conv3d weight column order)."""
    _req(src0, "patchify.src0")
    if src0.dim() != 4 or not src0.is_contiguous():
        raise GoalForceError("patchify.src0: expected contiguous [c,F,H,W]")
    c0, F, H, W = src0.shape
    c1 = 0
    if src1 is not None:
        _req(src1, "patchify.src1")
        if src1.dim() != 4 or not src1.is_contiguous() or src1.shape[1:] != src0.shape[1:]:
            raise GoalForceError("patchify.src1: expected contiguous [c1,F,H,W] matching src0")
        c1 = src1.shape[0]
    if kpad is None:
        kpad = -(-((c0 + c1) * 4) // 64) * 64
    out = torch.empty((F * (H // 2) * (W // 2), kpad), dtype=_BF16, device=src0.device)
    _lib.check(_lib.load().gf_patchify_im2col(_ptr(src0), c0, _ptr(src1), c1, _ptr(out), F, H, W, kpad,
                                              _stream(src0)), "gf_patchify_im2col")
    return out


def unpatchify(tokens, c, f, h, w):
    """[f*h*w, 4c] -> [c, f, 2h, 2w]."""
    _req(tokens, "unpatchify.tokens")
    if tokens.shape != (f * h * w, 4 * c) or not tokens.is_contiguous():
        raise GoalForceError(f"unpatchify.tokens: expected contiguous [{f * h * w}, {4 * c}]")
    out = torch.empty((c, f, 2 * h, 2 * w), dtype=_BF16, device=tokens.device)
    _lib.check(_lib.load().gf_unpatchify(_ptr(tokens), _ptr(out), c, f, h, w, _stream(tokens)), "gf_unpatchify")
    return out


def cfg_euler_step(latents, posi, nega, cfg_scale, dsigma):
    """In place: latents += (nega + cfg*(posi-nega)) * dsigma with bf16 rounding after every op."""
    if posi is None:
        raise GoalForceError("cfg_euler_step.posi: required")
    n = _flat("cfg_euler_step", latents=latents, posi=posi, nega=nega)
    _lib.check(_lib.load().gf_cfg_euler_step(_ptr(latents), _ptr(posi), _ptr(nega), float(cfg_scale), float(dsigma), n,
                                             _stream(latents)), "gf_cfg_euler_step")
    return latents


def act(x, kind: str):
    n = _flat("act", x=x)
    out = torch.empty_like(x)
    _lib.check(_lib.load().gf_act(_ptr(x), _ptr(out), n, {"silu": 0, "gelu_tanh": 1}[kind], _stream(x)), "gf_act")
    return out


def add(a, b, out=None):
    n = _flat("add", a=a, b=b)
    if out is None:
        out = torch.empty_like(a)
    _lib.check(_lib.load().gf_add_bf16(_ptr(a), _ptr(b), _ptr(out), n, _stream(a)), "gf_add_bf16")
    return out


def sub(a, b, out=None):
    """bf16(a - b), one rounding of the fp32 difference; `out` may be `a` or `b` (TeaCache's residual, teacache.py)."""
    n = _flat("sub", a=a, b=b, out=out)
    if out is None:
        out = torch.empty_like(a)
    _lib.check(_lib.load().gf_sub_bf16(_ptr(a), _ptr(b), _ptr(out), n, _stream(a)), "gf_sub_bf16")
    return out


def rel_l1(cur, prev):
    """(sum |bf16(cur - prev)|, sum |prev|) of two equal-sized bf16 tensors as Python floats: one single-block kernel (fp32
    sums in a fixed order, the same bits on every call) and ONE 8-byte read-back, which waits for the stream — dit.pad_run is
    the other place the forward does that."""
    n = _flat("rel_l1", cur=cur, prev=prev)
    if n == 0 or n % 8:
        raise GoalForceError(f"rel_l1: the element count must be a positive multiple of 8, got {n}")
    sums = torch.empty(2, dtype=torch.float32, device=cur.device)
    _lib.check(_lib.load().gf_rel_l1_bf16(_ptr(cur), _ptr(prev), n, _ptr(sums), _stream(cur)), "gf_rel_l1_bf16")
    s_diff, s_prev = sums.tolist()
    return s_diff, s_prev


def force_map(frames, H, W, channels, params, centers, clamp01, device):
    """Render the control-signal video [frames,H,W,3] bf16; blob arrays are torch tensors on `device`."""
    out = torch.empty((frames, H, W, 3), dtype=_BF16, device=device)
    n = int(channels.numel())
    if n:
        _req(channels, "force_map.channels", torch.int32)
        _req(params, "force_map.params", torch.float32)
        _req(centers, "force_map.centers", torch.float32)
        if params.shape != (n, 2) or centers.shape != (n, frames, 2) or not params.is_contiguous() \
                or not centers.is_contiguous():
            raise GoalForceError("force_map: params [n,2] / centers [n,frames,2] expected")
    _lib.check(_lib.load().gf_force_map(_ptr(out), frames, H, W, _ptr(channels) if n else None,
                                        _ptr(params) if n else None, _ptr(centers) if n else None, n,
                                        1 if clamp01 else 0, _stream(out)), "gf_force_map")
    return out


# ---------------------------------------------------------------------------------- VAE decoder kernels
def vae_prep_latent(z_slice, mean, inv_std, cpad=64):
    """z_slice: [C,T,H,W] bf16 view (any strides) -> channels-last [T,H,W,cpad], un-normalised."""
    _req(z_slice, "vae_prep_latent.z")
    _req(mean, "vae_prep_latent.mean")
    _req(inv_std, "vae_prep_latent.inv_std")
    C, T, H, W = z_slice.shape
    out = torch.empty((T, H, W, cpad), dtype=_BF16, device=z_slice.device)
    sc, st, sy, sx = z_slice.stride()
    _lib.check(_lib.load().gf_vae_prep_latent(_ptr(z_slice), sc, st, sy, sx, _ptr(mean), _ptr(inv_std), _ptr(out), C, T,
                                              H, W, cpad, _stream(z_slice)), "gf_vae_prep_latent")
    return out


def _conv_window(op, src, cache, upsample2x, downsample2, t_stride, t_off, t_out):
    """The gather of vae_im2col / vae_conv3d: src [T,H,W,C] contiguous (+ cache [2,H,W,C]) and the temporal window
    -> (mode, t_out, output pixels per frame); modes: see gf_vae_im2col."""
    _req(src, f"{op}.src")
    if src.dim() != 4 or not src.is_contiguous():
        raise GoalForceError(f"{op}.src must be contiguous [T,H,W,C]")
    T, H, W, C = src.shape
    if cache is not None:
        _req(cache, f"{op}.cache")
        if tuple(cache.shape) != (2, H, W, C) or not cache.is_contiguous():
            raise GoalForceError(f"{op}.cache must be contiguous [2,{H},{W},{C}]")
    mode = 1 if upsample2x else (2 if downsample2 else 0)
    if t_out is None:
        t_out = (T - t_off + t_stride - 1) // t_stride
    if t_off + (t_out - 1) * t_stride >= T:
        raise GoalForceError(f"{op}: temporal window exceeds the source")
    return mode, t_out, H * W * 4 if mode == 1 else ((H // 2) * (W // 2) if mode == 2 else H * W)


def _conv_resid(op, rows, bias, resid):
    """The epilogue operands of the VAE convolutions: bias bf16; resid [rows, >= N] with contiguous rows -> its row stride (0: none)."""
    if bias is not None:
        _req(bias, f"{op}.bias")
    if resid is None:
        return 0
    _mat(resid, f"{op}.resid")
    if resid.shape[0] != rows:
        raise GoalForceError(f"{op}.resid must be [{rows}, >= N] with contiguous rows")
    return resid.stride(0)


def vae_im2col(src, cache, kt, ks, kpad, upsample2x=False, downsample2=False, t_stride=1, t_off=0, t_out=None):
    """src [T,H,W,C] (+cache [2,H,W,C]) -> [T_out*Ho*Wo, kpad] patch matrix (modes: see gf_vae_im2col)."""
    mode, t_out, px = _conv_window("vae_im2col", src, cache, upsample2x, downsample2, t_stride, t_off, t_out)
    T, H, W, C = src.shape
    out = torch.empty((t_out * px, kpad), dtype=_BF16, device=src.device)
    _lib.check(_lib.load().gf_vae_im2col(_ptr(src), _ptr(cache), _ptr(out), t_out, H, W, C, kt, ks, mode, t_stride, t_off,
                                         kpad, _stream(src)), "gf_vae_im2col")
    return out


def vae_conv3d(src, cache, w, bias, kt, ks, upsample2x=False, downsample2=False, t_stride=1, t_off=0, t_out=None,
               resid=None, out=None, history_in_front=False):
    """Causal conv as one implicit GEMM (gf_conv3d_bf16): src [T,H,W,C] (+cache [2,H,W,C]) x w [N, kpad] -> [T_out*Ho*Wo, N].
    Same arguments as vae_im2col + gemm(epilogue BIAS / BIAS_RESID); bit-identical to that pair.
    history_in_front: src is frames [2:] of one contiguous [2+T,H,W,C] buffer whose first two frames hold the causal history
    (pass cache=None): the faster pointer-per-row gather."""
    mode, t_out, px = _conv_window("vae_conv3d", src, cache, upsample2x, downsample2, t_stride, t_off, t_out)
    T, H, W, C = src.shape
    if kt == 3:
        if history_in_front:
            if cache is not None or src.storage_offset() < 2 * H * W * C:
                raise GoalForceError("vae_conv3d: history_in_front needs cache=None and src = buffer[2:] of a [2+T,H,W,C] buffer")
        elif cache is None:
            raise GoalForceError("vae_conv3d: a temporal kernel needs its 2-frame cache (or history_in_front)")
    _mat(w, "vae_conv3d.w")
    n, k = w.shape
    out = _out(out, "vae_conv3d.out", t_out * px, n, src.device)
    ldr = _conv_resid("vae_conv3d", t_out * px, bias, resid)
    with _timed(PROFILE_CONV, t_out * px, n, C, kt, ks, mode, resid is not None):
        _lib.check(_lib.load().gf_conv3d_bf16(_ptr(src), _ptr(cache), _ptr(w), w.stride(0), _ptr(bias), _ptr(out), out.stride(0),
                                              T, t_out, H, W, C, kt, ks, mode, t_stride, t_off, n, k,
                                              EPI_BIAS if resid is None else EPI_BIAS_RESID, _ptr(resid), ldr, _stream(src)),
                   "gf_conv3d_bf16")
    return out


PADDED_CONV_CHANNELS = (192, 384)     # the levels whose 3x3x3 convolutions run on gf_conv3d_padded_bf16


def padded_conv_fits(T, H, W, C, history=True):
    """Whether gf_conv3d_padded_bf16 can take this shape: the zero-bordered buffer is addressed with 32-bit byte offsets (< 4 GiB) and
    its rows with 31-bit indices.  A production tile is far below (0.82 GB at the 192-channel level); an UNTILED 480 x 832 decode
    exceeds it at the 384 -> 192 resample convolution (6.3 GB) — such shapes stay on the implicit GEMM."""
    rows = (T + (2 if history else 0)) * (H + 2) * (W + 2)
    return C in PADDED_CONV_CHANNELS and rows * C * 2 < (1 << 32) and rows < (1 << 31)


def padded_activation(T, H, W, C, device, history=True):
    """A zero-bordered conv input [2 + T, H + 2, W + 2, C] (gf_conv3d_padded_bf16) and two views of it: the two history frames'
    interior [2, H, W, C] and the T frames' interior [T, H, W, C].  history=False (a per-frame 3x3 convolution, kt = 1):
    [T, H + 2, W + 2, C] and (buf, None, interior).  Zeroed once here; producers only ever write the interiors."""
    h = 2 if history else 0
    buf = torch.zeros((T + h, H + 2, W + 2, C), dtype=_BF16, device=device)
    return buf, (buf[:2, 1:H + 1, 1:W + 1] if history else None), buf[h:, 1:H + 1, 1:W + 1]


def vae_upsample2x_padded(x, buf):
    """nearest-exact 2x upsample of the contiguous x [T, H, W, C] into the interior of the zero-bordered `buf` [T, 2H + 2, 2W + 2, C]."""
    _req(x, "vae_upsample2x_padded.x")
    _req(buf, "vae_upsample2x_padded.buf")
    T, H, W, C = x.shape
    if not x.is_contiguous() or not buf.is_contiguous() or tuple(buf.shape) != (T, 2 * H + 2, 2 * W + 2, C):
        raise GoalForceError("vae_upsample2x_padded: x [T,H,W,C] contiguous, buf [T,2H+2,2W+2,C] contiguous")
    _lib.check(_lib.load().gf_vae_upsample2x_padded(_ptr(x), buf[0, 1, 1].data_ptr(), T, H, W, C, _stream(x)), "gf_vae_upsample2x_padded")
    return buf[:, 1:2 * H + 1, 1:2 * W + 1]


def vae_rmsnorm_silu_padded(x, gamma, buf, silu=True):
    """RMS_norm(+SiLU) of the contiguous x [T, H, W, C] into frames [2:] of the zero-bordered buffer `buf` [2 + T, H + 2, W + 2, C]."""
    _req(x, "vae_rmsnorm_silu_padded.x")
    _req(gamma, "vae_rmsnorm_silu_padded.gamma")
    _req(buf, "vae_rmsnorm_silu_padded.buf")
    T, H, W, C = x.shape
    if not x.is_contiguous() or not buf.is_contiguous() or tuple(buf.shape) != (T + 2, H + 2, W + 2, C) or gamma.numel() != C:
        raise GoalForceError("vae_rmsnorm_silu_padded: x [T,H,W,C] contiguous, buf [T+2,H+2,W+2,C] contiguous")
    interior = buf[2, 1, 1]
    _lib.check(_lib.load().gf_vae_rmsnorm_silu_padded(_ptr(x), _ptr(gamma), interior.data_ptr(), T, H, W, C, 1 if silu else 0, _stream(x)),
               "gf_vae_rmsnorm_silu_padded")
    return buf[2:, 1:H + 1, 1:W + 1]


def vae_conv3d_padded(buf, w, bias, resid=None, out=None, kt=3):
    """kt = 3: CausalConv3d 3x3x3 on the zero-bordered activation `buf` [2 + T, H + 2, W + 2, C] (frames 0, 1 = history); kt = 1: a
    3x3 convolution per frame on `buf` [T, H + 2, W + 2, C].  x w [N, >= 9 kt C] -> [T*H*W, N]; resid [T*H*W, >= N] is added after
    the bf16 rounding of conv + bias.  Bit-identical to vae_conv3d."""
    _req(buf, "vae_conv3d_padded.buf")
    if buf.dim() != 4 or not buf.is_contiguous() or kt not in (1, 3):
        raise GoalForceError("vae_conv3d_padded.buf must be contiguous [kt-1+T, H+2, W+2, C], kt = 1 or 3")
    T, H, W, C = buf.shape[0] - (kt - 1), buf.shape[1] - 2, buf.shape[2] - 2, buf.shape[3]
    _mat(w, "vae_conv3d_padded.w")
    n = w.shape[0]
    if w.shape[1] < 9 * kt * C:
        raise GoalForceError("vae_conv3d_padded.w must be [N, >= 9 kt C] with contiguous rows")
    out = _out(out, "vae_conv3d_padded.out", T * H * W, n, buf.device)
    ldr = _conv_resid("vae_conv3d_padded", T * H * W, bias, resid)
    with _timed(PROFILE_CONV, T * H * W, n, C, kt, 3, 3, resid is not None):      # mode 3 = the padded-layout direct kernel
        _lib.check(_lib.load().gf_conv3d_padded_bf16(_ptr(buf), _ptr(w), w.stride(0), _ptr(bias), _ptr(out), out.stride(0), T, H, W, C, n,
                                                     kt, EPI_BIAS if resid is None else EPI_BIAS_RESID, _ptr(resid), ldr, _stream(buf)),
                   "gf_conv3d_padded_bf16")
    return out


def vae_finish_latent(x, mean, inv_std, C):
    """x [rows, >=C] (conv1 output, channels-last) -> [rows, C] normalised mu."""
    _mat(x, "vae_finish_latent.x")
    out = torch.empty((x.shape[0], C), dtype=_BF16, device=x.device)
    _lib.check(_lib.load().gf_vae_finish_latent(_ptr(x), x.stride(0), _ptr(mean), _ptr(inv_std), _ptr(out), x.shape[0], C,
                                                _stream(x)), "gf_vae_finish_latent")
    return out


def vae_rmsnorm_silu(x, gamma, silu=True, out=None):
    """x [..., C] channels-last -> RMS_norm(+SiLU), same shape (into `out` if given: contiguous, same shape)."""
    _req(x, "vae_rmsnorm_silu.x")
    _req(gamma, "vae_rmsnorm_silu.gamma")
    if not x.is_contiguous() or gamma.numel() != x.shape[-1]:
        raise GoalForceError("vae_rmsnorm_silu: x must be contiguous and gamma match the channel dim")
    if out is None:
        out = torch.empty_like(x)
    else:
        _req(out, "vae_rmsnorm_silu.out")
        if out.shape != x.shape or not out.is_contiguous():
            raise GoalForceError("vae_rmsnorm_silu.out must be contiguous with the shape of x")
    C = x.shape[-1]
    _lib.check(_lib.load().gf_vae_rmsnorm_silu(_ptr(x), _ptr(gamma), _ptr(out), x.numel() // C, C, 1 if silu else 0,
                                               _stream(x)), "gf_vae_rmsnorm_silu")
    return out


def softmax_rows(x, scale, ldo, bias=None, nvalid=None):
    """out[r,:] = softmax(bf16(x[r,:]*scale + bias[r,:])) over the first nvalid columns; zero-padded to ldo columns."""
    _mat(x, "softmax_rows.x")
    ldb = 0
    if bias is not None:
        _mat(bias, "softmax_rows.bias")
        if bias.shape != x.shape:
            raise GoalForceError("softmax_rows.bias must match x")
        ldb = bias.stride(0)
    out = torch.empty((x.shape[0], ldo), dtype=_BF16, device=x.device)
    _lib.check(_lib.load().gf_softmax_rows(_ptr(x), x.stride(0), _ptr(bias), ldb, _ptr(out), ldo, x.shape[0], x.shape[1],
                                           x.shape[1] if nvalid is None else int(nvalid), float(scale), _stream(x)),
               "gf_softmax_rows")
    return out


def rowmax_neg(x, out_col):
    """out_col[r] = -max_c x[r, c] (bf16, exact): x [R, C] with contiguous rows, out_col a [R] VIEW (any stride) — a column of the
    augmented Q operand of the VAE attention's second score GEMM (gf_rowmax_neg_bf16)."""
    _mat(x, "rowmax_neg.x")
    _req(out_col, "rowmax_neg.out_col")
    if out_col.dim() != 1 or out_col.shape[0] != x.shape[0]:
        raise GoalForceError(f"rowmax_neg.out_col: expected [{x.shape[0]}]")
    _lib.check(_lib.load().gf_rowmax_neg_bf16(_ptr(x), x.stride(0), _ptr(out_col), out_col.stride(0) if out_col.shape[0] > 1 else 1,
                                              x.shape[0], x.shape[1], _stream(x)), "gf_rowmax_neg_bf16")
    return out_col


def transpose_pad(x, rpad):
    _mat(x, "transpose_pad.x")
    R, C = x.shape
    out = torch.empty((C, rpad), dtype=_BF16, device=x.device)
    _lib.check(_lib.load().gf_transpose_pad(_ptr(x), x.stride(0), _ptr(out), R, C, rpad, _stream(x)), "gf_transpose_pad")
    return out


def transpose_pad_batched(x, rpad):
    """x [B, R, C] (any batch / row strides, contiguous last dim) -> [B, C, rpad] (zero columns past R) in one launch."""
    _req(x, "transpose_pad_batched.x")
    if x.dim() != 3 or x.stride(2) != 1:
        raise GoalForceError("transpose_pad_batched.x must be 3-D with a contiguous last dim")
    B, R, C = x.shape
    out = torch.empty((B, C, rpad), dtype=_BF16, device=x.device)
    _lib.check(_lib.load().gf_transpose_pad_batched(_ptr(x), x.stride(1), x.stride(0), _ptr(out), C * rpad, R, C, rpad, B, _stream(x)),
               "gf_transpose_pad_batched")
    return out


def gemm_batched(a, w, out=None):
    """out[b] = a[b] @ w[b]^T for b < B in ONE launch (gf_gemm_bf16_batched): a [B, M, K], w [B, N, K], out [B, M, N] — views with any
    batch / row strides and a contiguous last dim (heads of a [L, H*d] tensor: t.view(L, H, d).permute(1, 0, 2)).  No bias / epilogue.
    The 8-wave kernel: bit-identical to B calls of gemm() under options(prefer_8wave=1) (for M >= 512 gemm() takes the 4-wave kernel, which sums the
    same products from a rotated K tile on: equal up to fp32 summation order)."""
    _req(a, "gemm_batched.a")
    _req(w, "gemm_batched.w")
    if a.dim() != 3 or w.dim() != 3 or a.stride(2) != 1 or w.stride(2) != 1 or a.shape[0] != w.shape[0] or a.shape[2] != w.shape[2]:
        raise GoalForceError("gemm_batched: a [B, M, K] and w [B, N, K] with contiguous last dims")
    B, M, K = a.shape
    N = w.shape[1]
    if out is None:
        out = torch.empty((B, M, N), dtype=_BF16, device=a.device)
    else:
        _req(out, "gemm_batched.out")
        if tuple(out.shape) != (B, M, N) or out.stride(2) != 1:
            raise GoalForceError(f"gemm_batched.out: expected [{B}, {M}, {N}] with a contiguous last dim")
    _lib.check(_lib.load().gf_gemm_bf16_batched(_ptr(a), a.stride(1), a.stride(0), _ptr(w), w.stride(1), w.stride(0), _ptr(out),
                                                out.stride(1), out.stride(0), M, N, K, B, _stream(a)), "gf_gemm_bf16_batched")
    return out


def vae_tile_blend(values, weight, tile, y0, x0, bounds, border):
    """values [nch,T,H,W], weight [H,W], tile [T,th,tw,tc>=nch] channels-last; bounds=(top,bottom,left,right)."""
    for n, t in (("values", values), ("weight", weight), ("tile", tile)):
        _req(t, f"vae_tile_blend.{n}")
        if not t.is_contiguous():
            raise GoalForceError(f"vae_tile_blend.{n} must be contiguous")
    nch, T, H, W = values.shape
    Tt, th, tw, tc = tile.shape
    if Tt != T or tuple(weight.shape) != (H, W):
        raise GoalForceError("vae_tile_blend: shape mismatch")
    _lib.check(_lib.load().gf_vae_tile_blend(_ptr(values), _ptr(weight), _ptr(tile), nch, T, th, tw, tc, H, W, y0, x0,
                                             int(bounds[0]), int(bounds[1]), int(bounds[2]), int(bounds[3]),
                                             border[0], border[1], _stream(values)), "gf_vae_tile_blend")


def vae_tile_finalize(values, weight, clamp=True):
    _lib.check(_lib.load().gf_vae_tile_finalize(_ptr(values), _ptr(weight), values.shape[0] * values.shape[1],
                                                weight.numel(), 1 if clamp else 0, _stream(values)), "gf_vae_tile_finalize")
    return values


def _window_value(op, value, weight):
    """The accumulators of a sliding-window blend: value [C, T, *spatial] bf16 (a leading batch dim of 1 is taken off) whose
    spatial dims are contiguous — C and T may be strided, a slice of a larger tensor — and weight [T] bf16 contiguous
    -> (value as [C, T, ...], C, T, HW, stride of C, stride of T)."""
    _req(value, f"{op}.value")
    if value.dim() == 5 and value.shape[0] == 1:
        value = value[0]
    if value.dim() < 3 or value.numel() == 0:
        raise GoalForceError(f"{op}.value: expected a non-empty [C, T, ...] (or [1, C, T, H, W]), got {tuple(value.shape)}")
    C, T = value.shape[:2]
    HW = math.prod(value.shape[2:])
    inner = 1
    for d in range(value.dim() - 1, 1, -1):
        if value.shape[d] != 1 and value.stride(d) != inner:
            raise GoalForceError(f"{op}.value: the dims after T must be contiguous")
        inner *= value.shape[d]
    sc, st = value.stride(0), value.stride(1)
    if st < HW or sc < (T - 1) * st + HW:
        raise GoalForceError(f"{op}.value: the [T, ...] planes of the channels overlap (strides {tuple(value.stride())})")
    _vec(weight, f"{op}.weight", T, required=True)
    return value, C, T, HW, sc, st


def window_blend(value, weight, win, t0, bounds, border):
    """One temporal window into the accumulators of TemporalTiler_BCTHW.run (gf_window_blend): value [C, T, ...] += win * mask,
    weight [T] += mask, every op rounded to bf16.  win [C, len, ...] (or [1, C, len, H, W]) is the window's prediction for frames
    t0 .. t0+len-1; bounds = (left, right): the window touches that end of the clip (no ramp there); border = size - stride."""
    value, C, T, HW, sc, st = _window_value("window_blend", value, weight)
    _req(win, "window_blend.win")
    if win.dim() == 5 and win.shape[0] == 1:
        win = win[0]
    if win.dim() != value.dim() or win.shape[0] != C or win.shape[2:] != value.shape[2:] or not win.is_contiguous():
        raise GoalForceError(f"window_blend.win: expected contiguous [{C}, len, {', '.join(map(str, value.shape[2:]))}], "
                             f"got {tuple(win.shape)}")
    _lib.check(_lib.load().gf_window_blend(_ptr(value), _ptr(weight), _ptr(win), C, T, HW, sc, st, int(t0), win.shape[1],
                                           int(bool(bounds[0])), int(bool(bounds[1])), int(border), _stream(value)),
               "gf_window_blend")


def window_finalize(value, weight):
    """In place: value[c, t] /= weight[t], one bf16 rounding, no clamp (gf_window_finalize); returns value."""
    v, C, T, HW, sc, st = _window_value("window_finalize", value, weight)
    _lib.check(_lib.load().gf_window_finalize(_ptr(v), _ptr(weight), C, T, HW, sc, st, _stream(v)), "gf_window_finalize")
    return value


# ---------------------------------------------------------------------------------- fp8 Linear (VRAM:115-151)


def quant_fp8_rowscale(x):
    """x [M,K] bf16 -> (x8 [M,K] float8_e4m3fn, scale_a [M] fp32) — gf_quant_fp8_rowscale."""
    _req(x, "quant_fp8_rowscale.x")
    xv, rows, dim, xs = _rows2d(x, "quant_fp8_rowscale.x")
    out = torch.empty((rows, dim), dtype=_FP8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().gf_quant_fp8_rowscale(_ptr(xv), _ptr(out), _ptr(scale), rows, dim, xs, dim, _stream(x)),
               "gf_quant_fp8_rowscale")
    return out, scale


def layernorm_modulate_fp8(x, weight=None, bias=None, scale1p=None, shift=None, eps=1e-6):
    """LayerNorm(+affine)(+modulate) straight into the fp8_linear input format: (x8 [M,K] float8_e4m3fn, scale_a [M] fp32) —
    gf_layernorm_modulate_fp8 at the DiT widths (the bf16 row never reaches HBM), elsewhere the two kernels it fuses; the same
    bits either way."""
    operands = _layernorm_operands("layernorm_modulate_fp8", x, weight, bias, scale1p, shift, widths=LN_QUANT_WIDTHS)
    if operands is None:
        return quant_fp8_rowscale(layernorm_modulate(x, weight=weight, bias=bias, scale1p=scale1p, shift=shift, eps=eps))
    xv, rows, dim, xs = operands
    out = torch.empty((rows, dim), dtype=_FP8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().gf_layernorm_modulate_fp8(_ptr(xv), _ptr(out), _ptr(scale), _ptr(weight), _ptr(bias), _ptr(scale1p),
                                                     _ptr(shift), rows, dim, xs, dim, float(eps), _stream(x)),
               "gf_layernorm_modulate_fp8")
    return out, scale


def cast_fp8(w):
    """bf16 -> float8_e4m3fn, elementwise (weights; unit scale)."""
    _req(w, "cast_fp8.w")
    if not w.is_contiguous() or w.numel() % 8:
        raise GoalForceError("cast_fp8: contiguous tensor with numel % 8 == 0 expected")
    out = torch.empty(w.shape, dtype=_FP8, device=w.device)
    _lib.check(_lib.load().gf_cast_fp8(_ptr(w), _ptr(out), w.numel(), _stream(w)), "gf_cast_fp8")
    return out


def quant_fp8_grad(x):
    """A gradient x [M,K] bf16 (rows may be strided) -> (x8 [M,K] float8_e4m3fn, scale [M] fp32, a power of two per row) —
    gf_quant_fp8_grad: x8 = e4m3(x / scale) with the division exact; an inf / NaN row gives scale NaN."""
    _req(x, "quant_fp8_grad.x")
    xv, rows, dim, xs = _rows2d(x, "quant_fp8_grad.x")
    out = torch.empty((rows, dim), dtype=_FP8, device=x.device)
    scale = torch.empty((rows,), dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().gf_quant_fp8_grad(_ptr(xv), _ptr(out), _ptr(scale), rows, dim, xs, dim, _stream(x)), "gf_quant_fp8_grad")
    return out, scale


def cast_fp8_t(w):
    """w [N,K] bf16 (contiguous rows) -> [K,N] float8_e4m3fn, cast_fp8(w).t() made in one pass — gf_cast_fp8_t; N % 128 == 0, K % 8 == 0."""
    _mat(w, "cast_fp8_t.w")
    N, K = w.shape
    out = torch.empty((K, N), dtype=_FP8, device=w.device)
    _lib.check(_lib.load().gf_cast_fp8_t(_ptr(w), w.stride(0), _ptr(out), N, N, K, _stream(w)), "gf_cast_fp8_t")
    return out


def gemm_fp8(a8, row_scale, w8, bias=None, epilogue=EPI_BIAS, resid=None, gate=None, out=None):
    """out[M,N] = epilogue((a8 @ w8^T) * row_scale[:,None] + bias) — gf_gemm_fp8."""
    if row_scale is None:
        raise GoalForceError("gemm_fp8.row_scale: required")
    return _gemm(a8, w8, row_scale, bias, epilogue, resid, gate, out)


FP8_LORA_RANK_PADS = (32, 64)     # the padded ranks gf_gemm_fp8_lora holds in its epilogue's registers


def gemm_fp8_lora_ok(M, N, K, rank_pad) -> bool:
    """Where gf_gemm_fp8_lora runs (gf_gemm_fp8_lora_ok, asked of the library: the option prefer_8wave is part of the answer)."""
    return bool(_lib.load().gf_gemm_fp8_lora_ok(M, N, K, rank_pad))


def gemm_fp8_lora(a8, row_scale, w8, bias, t, up, scale, epilogue=EPI_BIAS, resid=None, gate=None, out=None):
    """out[M,N] = epilogue(bf16(y0 + bf16(fp32(scale) * bf16(t[M,R] @ up[N,R]^T))), resid, gate) with y0 = bf16((a8 @ w8^T) * row_scale
    + bias): an fp8 Linear with one attached adapter on the bf16 input (t = gemm(x, down_pad)), the reference's
    AutoWrappedLinear.forward (VRAM:168-187).  One launch, gf_gemm_fp8_lora, where gf_gemm_fp8_lora_ok says so and
    option("fp8_lora_fused") is on; otherwise gemm_fp8(EPI_BIAS) into a new tensor and lora_up: the same bits by contract.
    `out` may be resid (None: a new tensor)."""
    op = "gemm_fp8_lora"
    if row_scale is None:
        raise GoalForceError(f"{op}.row_scale: required")
    av, M, K, lda, N, ldw = _linear_operands(a8, w8, row_scale)
    R = t.shape[-1]
    tv, ldt = _rows_like(t, f"{op}.t", M, R)
    Nu, ld_up = _weight(up, f"{op}.up", R)
    if Nu != N:
        raise GoalForceError(f"{op}.up: expected [{N}, {R}], got {tuple(up.shape)}")
    if R % 32 or not 32 <= R <= LORA_MAX_RANK:
        raise GoalForceError(f"{op}: padded rank {R}: expected a multiple of 32 in 32..{LORA_MAX_RANK}")
    scale = _lora_scale(op, "scale", scale)
    if not (option("fp8_lora_fused") and gemm_fp8_lora_ok(M, N, K, R) and 256 * max(lda, ldw) + K < 2 ** 31):
        y0 = gemm_fp8(a8, row_scale, w8, bias)
        return lora_up(y0, t, up, scale, epilogue=epilogue, resid=resid, gate=gate, out=y0 if out is None else out)
    if out is None:
        out = torch.empty((M, N), dtype=_BF16, device=a8.device)
    ov, ldo, resid, ldr = _gemm_result_operands(op, M, N, out, resid, gate, bias)
    with _timed(PROFILE_GEMM, M, N, K, int(epilogue)):
        _lib.check(_lib.load().gf_gemm_fp8_lora(_ptr(av), lda, _ptr(w8), ldw, _ptr(row_scale), _ptr(bias), _ptr(tv), ldt, _ptr(up), ld_up,
                                                R, scale, _ptr(ov), ldo, M, N, K, int(epilogue), _ptr(resid), ldr, _ptr(gate),
                                                _stream(a8)), "gf_gemm_fp8_lora")
    return out


# ---------------------------------------------------------------------------------- MXFP4 Linear (goalforce.h; no reference counterpart)


def quant_mxfp4(x):
    """x [M,K] bf16 (rows may be strided) -> (x4 [M,K/2] uint8 packed e2m1, scale [M,K/32] uint8 E8M0) — gf_quant_mxfp4; K % 32 == 0."""
    _req(x, "quant_mxfp4.x")
    xv, rows, dim, xs = _rows2d(x, "quant_mxfp4.x")
    if dim % 32:
        raise GoalForceError(f"quant_mxfp4.x: the row length {dim} must be a multiple of 32 (one E8M0 scale per 32 elements)")
    out = torch.empty((rows, dim // 2), dtype=torch.uint8, device=x.device)
    scale = torch.empty((rows, dim // 32), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().gf_quant_mxfp4(_ptr(xv), xs, _ptr(out), dim // 2, _ptr(scale), dim // 32, rows, dim, _stream(x)),
               "gf_quant_mxfp4")
    return out, scale


def layernorm_modulate_mxfp4(x, weight=None, bias=None, scale1p=None, shift=None, eps=1e-6):
    """LayerNorm(+affine)(+modulate) straight into the fp4 Linear's input format: (x4 [M,K/2] uint8 packed e2m1, scale [M,K/32] uint8
    E8M0) — gf_layernorm_modulate_mxfp4 at the DiT widths (the bf16 row never reaches HBM), elsewhere the two kernels it fuses; the
    same bits either way."""
    operands = _layernorm_operands("layernorm_modulate_mxfp4", x, weight, bias, scale1p, shift, widths=LN_QUANT_WIDTHS)
    if operands is None:
        return quant_mxfp4(layernorm_modulate(x, weight=weight, bias=bias, scale1p=scale1p, shift=shift, eps=eps))
    xv, rows, dim, xs = operands
    out = torch.empty((rows, dim // 2), dtype=torch.uint8, device=x.device)
    scale = torch.empty((rows, dim // 32), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().gf_layernorm_modulate_mxfp4(_ptr(xv), _ptr(out), _ptr(scale), _ptr(weight), _ptr(bias), _ptr(scale1p),
                                                       _ptr(shift), rows, dim, xs, dim // 2, dim // 32, float(eps), _stream(x)),
               "gf_layernorm_modulate_mxfp4")
    return out, scale


def _mxfp4_operands(a4, a_scale, w4, w_scale):
    """The four operands of an fp4 GEMM, checked in gemm_mxfp4's words -> (M, N, K, ldw)."""
    _mat(a4, "mxfp4 linear: activation", torch.uint8)
    M, K2 = a4.shape
    K = 2 * K2
    N, ldw = _weight(w4, "mxfp4 linear: weight", K2, torch.uint8)
    for t, name, rows in ((a_scale, "mxfp4 linear: activation scales", M), (w_scale, "mxfp4 linear: weight scales", N)):
        if t is None:
            raise GoalForceError(f"{name}: required")
        _mat(t, name, torch.uint8)
        if tuple(t.shape) != (rows, K // 32):
            raise GoalForceError(f"{name}: expected [{rows}, {K // 32}], got {tuple(t.shape)}")
    return M, N, K, ldw


def gemm_mxfp4_q4(a4, a_scale, w4, w_scale, bias=None, epilogue=EPI_BIAS):
    """(c4 [M,N/2], c_scale [M,N/32]) = quant_mxfp4(gemm_mxfp4(a4, a_scale, w4, w_scale, bias, epilogue)) in one launch —
    gf_gemm_mxfp4_q4: the GEMM's epilogue quantises its finished bf16 values, which never reach HBM; the same bits as the two calls.
    N % 32 == 0 and an epilogue without a second operand (EPI_BIAS, EPI_BIAS_GELU_TANH, EPI_BIAS_SILU); otherwise gemm_mxfp4's rules."""
    if int(epilogue) not in (EPI_BIAS, EPI_BIAS_GELU_TANH, EPI_BIAS_SILU):
        raise GoalForceError(f"gemm_mxfp4_q4: epilogue {int(epilogue)} is not one of EPI_BIAS, EPI_BIAS_GELU_TANH, EPI_BIAS_SILU: an epilogue "
                             "with a residual operand is not quantised in the GEMM (use gemm_mxfp4 + quant_mxfp4)")
    if torch.is_tensor(w4) and w4.dim() == 2 and w4.shape[0] % 32:
        raise GoalForceError(f"gemm_mxfp4_q4: N = {w4.shape[0]} output features must be a multiple of 32 (one E8M0 scale per 32 columns)")
    M, N, K, ldw = _mxfp4_operands(a4, a_scale, w4, w_scale)
    _vec(bias, "gemm_mxfp4_q4.bias", N)
    c4 = torch.empty((M, N // 2), dtype=torch.uint8, device=a4.device)
    c_scale = torch.empty((M, N // 32), dtype=torch.uint8, device=a4.device)
    if M == 0:                       # nothing to compute (an empty tensor has no address to hand over)
        return c4, c_scale
    with _timed(PROFILE_GEMM, M, N, K, int(epilogue)):
        _lib.check(_lib.load().gf_gemm_mxfp4_q4(_ptr(a4), a4.stride(0), _ptr(a_scale), a_scale.stride(0), _ptr(w4), ldw, _ptr(w_scale),
                                                w_scale.stride(0), _ptr(bias), _ptr(c4), N // 2, _ptr(c_scale), N // 32, M, N, K,
                                                int(epilogue), _stream(a4)), "gf_gemm_mxfp4_q4")
    return c4, c_scale


def gemm_mxfp4(a4, a_scale, w4, w_scale, bias=None, epilogue=EPI_BIAS, resid=None, gate=None, out=None):
    """out[M,N] = epilogue(bf16(deq(a4, a_scale) @ deq(w4, w_scale)^T + bias)) — gf_gemm_mxfp4.  a4 [M,K/2] / w4 [N,K/2] uint8 packed
    e2m1, a_scale [M,K/32] / w_scale [N,K/32] uint8 E8M0 (ops.quant_mxfp4); K % 256 == 0.  out / resid / gate / bias as in _gemm."""
    M, N, K, ldw = _mxfp4_operands(a4, a_scale, w4, w_scale)
    if out is None:
        out = torch.empty((M, N), dtype=_BF16, device=a4.device)
    ov, ldc, resid, ldr = _gemm_result_operands("gemm_mxfp4", M, N, out, resid, gate, bias)
    if M == 0:                       # nothing to compute (an empty tensor has no address to hand over)
        return out
    with _timed(PROFILE_GEMM, M, N, K, int(epilogue)):
        _lib.check(_lib.load().gf_gemm_mxfp4(_ptr(a4), a4.stride(0), _ptr(a_scale), a_scale.stride(0), _ptr(w4), ldw, _ptr(w_scale),
                                             w_scale.stride(0), _ptr(bias), _ptr(ov), ldc, M, N, K, int(epilogue), _ptr(resid), ldr,
                                             _ptr(gate), _stream(a4)), "gf_gemm_mxfp4")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# backward / training ops (gf_backward.hip, gf_attention_bwd.hip)
def _f32(t, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise GoalForceError(f"{name}: expected a contiguous fp32 CUDA tensor")
    return t


def _f32n(t, name, n: int, at_least=False):
    """An fp32 operand of the backward kernels (column accumulator, RoPE table): contiguous, n elements (or at least n); None passes."""
    if t is None:
        return None
    _f32(t, name)
    if t.numel() != n and not (at_least and t.numel() > n):
        raise GoalForceError(f"{name}: expected {'at least ' if at_least else ''}{n} fp32 elements, got {t.numel()}")
    return t


def _rows_like(t, name: str, rows: int, dim: int):
    """A second [rows, dim] operand of a row kernel (a row stride of its own is fine) -> (tensor, row stride)."""
    _req(t, name)
    v, r, d, stride = _rows2d(t, name)
    if (r, d) != (rows, dim):
        raise GoalForceError(f"{name}: expected [{rows}, {dim}] like the first operand, got {tuple(t.shape)}")
    return v, stride


def layernorm_bwd(x, dy, g=None, dg_acc=None, db_acc=None, eps=1e-6):
    """dx of LayerNorm with y = xhat*g (+b) (g = affine weight, or 1+scale, or None); fp32 [dim] accumulators optional."""
    _req(x, "layernorm_bwd.x")
    xv, rows, dim, xs = _rows2d(x, "layernorm_bwd.x")
    dv, ds = _rows_like(dy, "layernorm_bwd.dy", rows, dim)
    _vec(g, "layernorm_bwd.g", dim)
    _f32n(dg_acc, "layernorm_bwd.dg_acc", dim)
    _f32n(db_acc, "layernorm_bwd.db_acc", dim)
    dx = torch.empty((rows, dim), dtype=_BF16, device=x.device)
    _lib.check(_lib.load().gf_layernorm_bwd(_ptr(xv), xs, _ptr(dv), ds, _ptr(g), _ptr(dx), dim, _ptr(dg_acc), _ptr(db_acc),
                                            rows, dim, float(eps), _stream(x)), "gf_layernorm_bwd")
    return dx.view(x.shape)


def rmsnorm_rope_bwd(x_pre, dy, weight, cos=None, sin=None, head_dim=128, eps=1e-6, dw_acc=None):
    """dx of y = rope(x * rsqrt(mean(x^2) + eps) * weight) for the PRE-norm x; cos / sin fp32 [rows, head_dim/2] or both None (no
    rotation); dw_acc fp32 [dim] optional."""
    _req(x_pre, "rmsnorm_rope_bwd.x")
    xv, rows, dim, xs = _rows2d(x_pre, "rmsnorm_rope_bwd.x")
    dv, ds = _rows_like(dy, "rmsnorm_rope_bwd.dy", rows, dim)
    _vec(weight, "rmsnorm_rope_bwd.weight", dim, required=True)
    head_dim = int(head_dim)
    if (cos is None) != (sin is None):
        raise GoalForceError("rmsnorm_rope_bwd: cos and sin go together")
    if head_dim <= 0 or head_dim % 8 or dim % head_dim:
        raise GoalForceError(f"rmsnorm_rope_bwd: dim={dim} head_dim={head_dim} unsupported (head_dim a multiple of 8 that divides dim)")
    _f32n(cos, "rmsnorm_rope_bwd.cos", rows * (head_dim // 2), at_least=True)
    _f32n(sin, "rmsnorm_rope_bwd.sin", rows * (head_dim // 2), at_least=True)
    _f32n(dw_acc, "rmsnorm_rope_bwd.dw_acc", dim)
    dx = torch.empty((rows, dim), dtype=_BF16, device=x_pre.device)
    _lib.check(_lib.load().gf_rmsnorm_rope_bwd(_ptr(xv), xs, _ptr(dv), ds, _ptr(weight), _ptr(cos), _ptr(sin), _ptr(dx), dim,
                                               _ptr(dw_acc), rows, dim, head_dim, float(eps), _stream(x_pre)),
               "gf_rmsnorm_rope_bwd")
    return dx.view(x_pre.shape)


def colsum(a, b=None, gate=None, acc=None):
    """acc[n] += sum_r a[r,n]*(b[r,n] or 1); with `gate` also returns bf16(a*gate) (else None)."""
    _req(a, "colsum.a")
    av, rows, cols, lda = _rows2d(a, "colsum.a")
    bv, ldb = (None, 0) if b is None else _rows_like(b, "colsum.b", rows, cols)
    _vec(gate, "colsum.gate", cols)
    _f32n(acc, "colsum.acc", cols)
    if gate is None and acc is None:
        raise GoalForceError("colsum: nothing to compute (neither acc nor gate given)")
    out = None if gate is None else torch.empty((rows, cols), dtype=_BF16, device=a.device)
    _lib.check(_lib.load().gf_colsum(_ptr(av), lda, _ptr(bv), ldb, _ptr(gate), _ptr(out), cols, _ptr(acc), rows, cols,
                                     _stream(a)), "gf_colsum")
    return None if out is None else out.view(a.shape)


def act_bwd(u, df, kind: str):
    n = _flat("act_bwd", u=u, df=df)
    du = torch.empty_like(u)
    _lib.check(_lib.load().gf_act_bwd(_ptr(u), _ptr(df), _ptr(du), n, {"gelu_tanh": 0, "silu": 1}[kind], _stream(u)), "gf_act_bwd")
    return du


def mse_loss(pred, target, weight=1.0, want_grad=True):
    """(loss fp32 [1] = weight*mean((pred-target)^2), dpred bf16 or None)."""
    n = _flat("mse_loss", pred=pred, target=target)
    loss = torch.empty((1,), dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    _lib.check(_lib.load().gf_mse_loss(_ptr(pred), _ptr(target), None if dpred is None else _ptr(dpred), _ptr(loss),
                                       n, float(weight), _stream(pred)), "gf_mse_loss")
    return loss, dpred


def adamw_step(param, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0):
    n = _flat("adamw_step", param=param, grad=grad)
    _lib.check(_lib.load().gf_adamw_step(_ptr(param), _ptr(grad), _ptr(_f32(exp_avg, "exp_avg")),
                                         _ptr(_f32(exp_avg_sq, "exp_avg_sq")), n, float(lr), float(betas[0]),
                                         float(betas[1]), float(eps), float(weight_decay), int(step), float(grad_scale),
                                         _stream(param)), "gf_adamw_step")
    # the kernel wrote through the raw pointer: tell torch, so that everything derived from the old values (K-padded
    # patch weights, fp8 copies, the all-zero flag of a ControlNet — dit.param_key) is rebuilt on its next use
    torch.autograd.graph.increment_version(param)


def f32_to_bf16(acc):
    _f32(acc, "f32_to_bf16.acc")
    out = torch.empty(acc.shape, dtype=_BF16, device=acc.device)
    _lib.check(_lib.load().gf_f32_to_bf16(_ptr(acc), _ptr(out), acc.numel(), _stream(acc)), "gf_f32_to_bf16")
    return out


def sumsq(x, acc):
    """acc[0] += sum(x^2) over a contiguous bf16 tensor (fp32 accumulate)."""
    _lib.check(_lib.load().gf_sumsq(_ptr(x), _flat("sumsq", x=x), _ptr(_f32(acc, "sumsq.acc")), _stream(x)), "gf_sumsq")
