"""References for the block-sparse self-attention tests (test_sparse_attention_cpu.py / _gpu.py): the token-level restatement of
FrameWindow, the fp64 masked attention and masked SelfAttention, and the key gather behind the bit-identity bar."""
import math

import torch
import torch.nn.functional as F

QB, KB = 256, 64            # query rows per map row, keys per tile (kernel 3's workgroup and key tile)


def frame_window_by_tokens(grid, window, sink_frames):
    """FrameWindow's definition taken literally, token by token: token i may see token j iff |frame(i) - frame(j)| <= window or
    frame(j) < sink_frames; (b, t) is selected iff ANY token of query block b may see ANY token of tile t.  Small grids only."""
    f, h, w = grid
    S = f * h * w
    frame = torch.arange(S) // (h * w)
    see = ((frame[:, None] - frame[None, :]).abs() <= window) | (frame[None, :] < sink_frames)        # [S, S]
    nqb, nt = -(-S // QB), -(-S // KB)
    out = torch.zeros((nqb, nt), dtype=torch.bool)
    for b in range(nqb):
        for t in range(nt):
            out[b, t] = bool(see[QB * b:QB * b + QB, KB * t:KB * t + KB].any())
    return out


def token_mask(block_mask, sq, skv):
    """[n_qblocks, n_tiles] bool -> [sq, skv] bool: every query of a block sees every key of its selected tiles."""
    return block_mask.repeat_interleave(QB, 0)[:sq].repeat_interleave(KB, 1)[:, :skv]


def masked_attention_fp64(q, k, v, num_heads, block_masks, head_map=None, scale=None):
    """softmax over the selected keys only, fp64, full tensors: q [Sq, H*d], k / v [Skv, H*d]; block_masks [n_maps, nqb, nt]
    (or one [nqb, nt]); head h uses map head_map[h] (None: map 0).  Returns (out [Sq, H*d], log2-domain lse [Sq, H])."""
    if block_masks.dim() == 2:
        block_masks = block_masks[None]
    sq, skv, d = q.shape[0], k.shape[0], q.shape[1] // num_heads
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    out = torch.empty((sq, num_heads * d), dtype=torch.float64)
    lse = torch.empty((sq, num_heads), dtype=torch.float64)
    for h in range(num_heads):
        m = token_mask(block_masks[0 if head_map is None else int(head_map[h])], sq, skv)
        cols = slice(h * d, (h + 1) * d)
        s = (q[:, cols].double() @ k[:, cols].double().T) * scale
        s = s.masked_fill(~m, -math.inf)
        out[:, cols] = torch.softmax(s, dim=-1) @ v[:, cols].double()
        lse[:, h] = torch.logsumexp(s, dim=-1) / math.log(2.0)
    return out, lse


def gather_rows(x, tiles, kv_len):
    """The rows of x [kv_len, C] that belong to the 64-row tiles `tiles`, concatenated in that order (a ragged last tile stays ragged)."""
    idx = torch.cat([torch.arange(KB * int(t), min(KB * int(t) + KB, kv_len)) for t in tiles]).to(x.device)
    return x.index_select(0, idx).contiguous()


def dense_kernel3(ops, q, k, v, num_heads, scale=None):
    """gf_transpose_v32 + gf_flash_attn_fwd_vt32 (the dense kernel 3) on exactly these operands, whatever the key count (ops.flash_attn
    would send fewer than VT_MIN_KV keys to kernel 2): (out, lse)."""
    from goal_force_amd import _lib
    sq, skv = q.shape[0], k.shape[0]
    out = torch.empty((sq, num_heads * 128), dtype=torch.bfloat16, device=q.device)
    lse = torch.empty((sq, num_heads), dtype=torch.float32, device=q.device)
    ops._vt_attn(_lib.load(), q, k, v, None, out, lse, sq, skv, num_heads, 128, 1.0 / math.sqrt(128) if scale is None else scale, True)
    return out, lse


def rope_complex(freqs3, f, h, w):
    """The reference's complex rotary table [S, d/2] of a token grid (what RopeTable.from_grid builds its cos / sin from)."""
    return torch.cat([freqs3[0][:f].view(f, 1, 1, -1).expand(f, h, w, -1), freqs3[1][:h].view(1, h, 1, -1).expand(f, h, w, -1),
                      freqs3[2][:w].view(1, 1, w, -1).expand(f, h, w, -1)], dim=-1).reshape(f * h * w, -1)


def self_attention_fp64(x, freqs, sd, num_heads, eps, block_mask=None):
    """SelfAttention.forward (DIT:124-147) in fp64 throughout on the module's bf16 weights `sd` ("q.weight", ..., "norm_q.weight"),
    x [S, D], freqs complex [S, d/2]; block_mask [nqb, nt]: the softmax is taken over the selected keys only."""
    xd = x.double()

    def lin(n, t):
        return F.linear(t, sd[n + ".weight"].double(), sd[n + ".bias"].double())

    def norm(t, w):
        return t * torch.rsqrt(t.pow(2).mean(dim=-1, keepdim=True) + eps) * w.double()

    def rope(t):
        tc = torch.view_as_complex(t.reshape(t.shape[0], num_heads, -1, 2).contiguous())
        return torch.view_as_real(tc * freqs.to(torch.complex128)[:, None, :]).flatten(1)

    q, k, v = rope(norm(lin("q", xd), sd["norm_q.weight"])), rope(norm(lin("k", xd), sd["norm_k.weight"])), lin("v", xd)
    S = x.shape[0]
    mask = torch.ones((-(-S // QB), -(-S // KB)), dtype=torch.bool) if block_mask is None else block_mask
    a, _ = masked_attention_fp64(q, k, v, num_heads, mask)
    return lin("o", a)
