"""Torch restatement of the SageAttention backend's arithmetic (gf_sage_attention.hip, include/goalforce.h), the yardstick of
tests/test_sage_attention_*.py.  Everything is per head on [S, heads*128] tensors; it runs on whichever device its inputs live.

  K smoothing   k~ = fp32(k) - mu (mu: the kernel's own per-channel mean, handed in: an fp32 mean summed in another order
                is not bit-reproducible)
  Q, K~ -> int8 one fp32 scale per (head, block of 32 query rows / 64 keys from row 0): scale = amax / 127,
                code = rne(x * (127 / amax)) clamped to +-127; an all-zero block: scale 0, codes 0
  V -> e4m3fn   one scale per (head, channel) over all keys: scale = amax / 448, code = e4m3fn_rne(v * (448 / amax))
  tiny blocks   where 127 / amax (448 / amax) is not finite in fp32 (a non-zero amax below ~3.7e-37 / 1.3e-36): the reciprocal is
                FLT_MAX and the scale 2^-128 = fp32(1 / FLT_MAX) (include/goalforce.h) — no 0 x inf = NaN
  scores        s = fp32(float(int32 dot) * w), w = fp32(fp32(s_q s_k) * c), c = fp32(fp32(scale) * fp32(log2 e))
  softmax       keys in index order in tiles of T; running maximum m per row, moved when a tile's maximum exceeds it by more than
                tau (tau = 0: whenever it rises); P = e4m3fn(exp2(s - m + e)) (needs 2^(tau + e) <= 448); l = sum of that P;
                acc = sum P V_code — fp64 sums of exact products; O = bf16(acc / l * v_scale)
"""
from __future__ import annotations

import math

import numpy as np
import torch

HD = 128
QBLK, KBLK = 32, 64
E4M3_MAX = 448.0
FLT_MAX = float(np.finfo(np.float32).max)
TINY_SCALE = 2.0 ** -128


def _inv_scale(amax: torch.Tensor, top: float):
    """(reciprocal, scale) of a block's amax for the code range `top`: top / amax and amax / top; 0 and 0 for an all-zero block;
    FLT_MAX and 2^-128 where top / amax overflows fp32 (the header's tiny-block rule)."""
    top_t = torch.tensor(top, device=amax.device)
    r = top_t / amax
    tiny = (amax > 0) & ~(r <= FLT_MAX)
    inv = torch.where(amax > 0, torch.where(tiny, torch.full_like(r, FLT_MAX), r), torch.zeros_like(amax))
    return inv, torch.where(tiny, torch.full_like(r, TINY_SCALE), amax / top_t)


def softmax_factor(scale: float) -> float:
    """c = fp32(fp32(scale) x fp32(log2 e)) — the launcher's `scale * 1.4426950408889634f`."""
    return float(np.float32(np.float32(scale) * np.float32(1.4426950408889634)))


def _heads(x: torch.Tensor, num_heads: int) -> torch.Tensor:
    """[S, H*128] -> [H, S, 128] fp32."""
    return x.float().reshape(x.shape[0], num_heads, HD).transpose(0, 1)


def quant_int8(x: torch.Tensor, blk: int):
    """x [H, S, 128] fp32 -> (codes int8 [H, S, 128], scales fp32 [H, ceil(S / blk)])."""
    h, s, _ = x.shape
    nb = -(-s // blk)
    xp = torch.zeros((h, nb * blk, HD), dtype=torch.float32, device=x.device)
    xp[:, :s] = x
    amax = xp.reshape(h, nb, blk * HD).abs().amax(dim=2)                            # [H, nb]
    inv, scale = _inv_scale(amax, 127.0)
    codes = torch.round(xp * inv.repeat_interleave(blk, dim=1)[:, :, None]).clamp(-127, 127)   # fp32 product, round half to even
    return codes[:, :s].to(torch.int8), scale


def quant_q(q: torch.Tensor, num_heads: int):
    return quant_int8(_heads(q, num_heads), QBLK)


def quant_k(k: torch.Tensor, num_heads: int, mu: torch.Tensor):
    """mu [H, 128] fp32 (the kernel's)."""
    return quant_int8(_heads(k, num_heads) - mu.float().reshape(num_heads, 1, HD), KBLK)


def quant_v(v: torch.Tensor, num_heads: int):
    """-> (codes float8_e4m3fn [H, S, 128], scales fp32 [H, 128])."""
    x = _heads(v, num_heads)
    amax = x.abs().amax(dim=1)                                                      # [H, 128]
    inv, scale = _inv_scale(amax, E4M3_MAX)
    return (x * inv[:, None, :]).to(torch.float8_e4m3fn), scale


def vt_position(kv_len: int, device=None) -> torch.Tensor:
    """Position of every key inside the kernel's V^T rows: 128-key slices, key k of a slice at 32 ((k >> 2) & 3) + 4 (k >> 4) + (k & 3)."""
    key = torch.arange(kv_len, device=device)
    kl = key % 128
    return key - kl + 32 * ((kl >> 2) & 3) + 4 * (kl >> 4) + (kl & 3)


def attention(q, k, v, num_heads: int, mu: torch.Tensor, scale: float | None = None, T: int = 128, tau: float = 0.0, e: float = 8.0,
              rows=None, quantize: bool = True) -> torch.Tensor:
    """The backend's output [len(rows) or Sq, H*128] bf16.  q [Sq, H*128], k / v [Skv, H*128] bf16; mu the kernel's K mean; (T, tau, e)
    the kernel's tile, rescale threshold and exponent offset; rows: optional query-row indices (the quantisation still sees every row).
    quantize=False: the same tiles, smoothing and online softmax with every rounding left out (fp64 throughout; the self-check)."""
    assert 2.0 ** (tau + e) <= E4M3_MAX, "P would leave e4m3fn"
    scale = 1.0 / math.sqrt(HD) if scale is None else scale
    if quantize:
        c = torch.tensor(softmax_factor(scale), dtype=torch.float32)
        q8, sq = quant_q(q, num_heads)
        k8, sk = quant_k(k, num_heads, mu)
        v8, sv = quant_v(v, num_heads)
    else:
        c = torch.tensor(scale * math.log2(math.e), dtype=torch.float64)
        q8 = q.double().reshape(q.shape[0], num_heads, HD).transpose(0, 1)
        k8 = k.double().reshape(k.shape[0], num_heads, HD).transpose(0, 1) - mu.double().reshape(num_heads, 1, HD)
        v8 = v.double().reshape(v.shape[0], num_heads, HD).transpose(0, 1)
        sq = torch.ones((num_heads, -(-q.shape[0] // QBLK)), dtype=torch.float64, device=q.device)
        sk = torch.ones((num_heads, -(-k.shape[0] // KBLK)), dtype=torch.float64, device=q.device)
        sv = torch.ones((num_heads, HD), dtype=torch.float64, device=q.device)
    rnd = (lambda t: t.float()) if quantize else (lambda t: t)
    dev = q8.device
    rows = torch.arange(q.shape[0], device=dev) if rows is None else torch.as_tensor(rows, device=dev)
    skv = k.shape[0]
    qd = q8[:, rows].double()                                                       # [H, R, 128]
    wq = sq[:, rows // QBLK]                                                        # [H, R]
    kd, vd = k8.double(), v8.double()
    m = torch.full((num_heads, len(rows)), -math.inf, dtype=torch.float64, device=dev)
    l = torch.zeros((num_heads, len(rows)), dtype=torch.float64, device=dev)
    acc = torch.zeros((num_heads, len(rows), HD), dtype=torch.float64, device=dev)
    keys = torch.arange(skv, device=dev)
    for t0 in range(0, skv, T):
        t1 = min(skv, t0 + T)
        dot = qd @ kd[:, t0:t1].transpose(1, 2)                                     # exact integers
        w = rnd((wq[:, :, None] * sk[:, keys[t0:t1] // KBLK][:, None, :]) * c.to(dev))   # fp32(fp32(s_q s_k) c)
        s = (rnd(dot) * w).double()                                                 # fp32 scores
        mt = s.amax(dim=2)
        move = mt > m + tau
        m_new = torch.where(move, torch.maximum(m, mt), m)
        alpha = torch.exp2(m - m_new)
        alpha = torch.where(torch.isinf(m) & torch.isinf(m_new), torch.ones_like(alpha), alpha)
        acc *= alpha[:, :, None]
        l *= alpha
        m = m_new
        off = rnd(e - rnd(m)).double()                                              # fp32(e - m), as the kernel's FMA addend
        x = rnd(dot * w.double() + off[:, :, None]).double()                        # fp32(dot w + (e - m)): the kernel's one FMA
        p = torch.exp2(x).float().to(torch.float8_e4m3fn).double() if quantize else torch.exp2(x)
        l += p.sum(dim=2)
        acc += p @ vd[:, t0:t1]
    o = acc / l[:, :, None] * sv.double()[:, None, :]
    o = o.transpose(0, 1).reshape(len(rows), num_heads * HD)
    return o.to(torch.bfloat16) if quantize else o


def attention_fp64(q, k, v, num_heads: int, scale: float | None = None, rows=None) -> torch.Tensor:
    """Exact softmax attention in fp64 on the bf16 inputs (the error yardstick)."""
    scale = 1.0 / math.sqrt(HD) if scale is None else scale
    qh = q.double().reshape(q.shape[0], num_heads, HD).transpose(0, 1)
    if rows is not None:
        qh = qh[:, torch.as_tensor(rows, device=q.device)]
    kh = k.double().reshape(k.shape[0], num_heads, HD).transpose(0, 1)
    vh = v.double().reshape(v.shape[0], num_heads, HD).transpose(0, 1)
    p = torch.softmax((qh @ kh.transpose(1, 2)) * scale, dim=-1)
    return (p @ vh).transpose(0, 1).reshape(qh.shape[1], num_heads * HD)
