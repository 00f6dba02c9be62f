"""SageAttention backend on the GPU (gf_sage_attention.hip): the quantisation passes bit for bit against tests/sage_oracle.py, the
attention against the oracle run with the kernel's (T, tau, e), its error from fp64 against the oracle's, the module switch, the
`sageattn` drop-in and head parallelism."""
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import gen_inputs as gi
import sage_oracle as so

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SHAPES = [1, 31, 32, 33, 63, 64, 65, 2047, 4097]
# kernel vs oracle: both round the output to bf16 once, the kernel from fp32 and the oracle from fp64 sums; where the two values straddle
# a rounding boundary they land one bf16 ulp (2^-8 relative) apart, and an exp2 one fp32 ulp apart can move a P across an e4m3 boundary.
# Measured 1.4e-4 .. 2.1e-4 rel-L2 on these shapes; the bar is 5e-4, 75 x below the recipe's own error from fp64 (3.8e-2 at logit std 1).
BAR = 5e-4


def _qkv(sq, skv, heads, seed=0, std=1.0, width=None):
    """q, k, v on the GPU; `width` > heads*128: column slices of wider tensors (row stride > heads*128)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = width or heads * 128
    q = (torch.randn((sq, w), generator=g, device="cuda") * std).to(BF)
    k = (torch.randn((skv, w), generator=g, device="cuda") + 0.7 * torch.randn((1, w), generator=g, device="cuda")).to(BF)
    v = (torch.randn((skv, w), generator=g, device="cuda") + 0.3).to(BF)
    c0 = w - heads * 128
    return q[:, c0:], k[:, c0:], v[:, c0:]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _sage():
    from goal_force_amd import ops
    return ops


@pytest.mark.parametrize("heads,width", [(1, None), (5, None), (40, None), (2, 5 * 128)])
def test_quant_kernels_bit_identical_to_oracle(heads, width):
    ops = _sage()
    for s in SHAPES + ([32760] if heads == 40 else []):
        q, k, v = _qkv(s, s, heads, seed=s, width=width)
        mu = ops.sage_k_mean(k, heads)
        ref_mu = k.double().reshape(s, heads, 128).mean(0)
        assert float((mu.double() - ref_mu).abs().max()) <= 1e-6 * float(k.float().abs().max()), s
        q8, qs = ops.sage_quant_q(q, heads)
        rq8, rqs = so.quant_q(q, heads)
        assert torch.equal(q8.reshape(s, heads, 128).transpose(0, 1), rq8) and torch.equal(qs, rqs), ("q", s)
        k8, ks, _ = ops.sage_quant_k(k, heads, mu)
        rk8, rks = so.quant_k(k, heads, mu)
        nb = rks.shape[1]
        assert torch.equal(k8[:s].reshape(s, heads, 128).transpose(0, 1), rk8) and torch.equal(ks[:, :nb], rks), ("k", s)
        assert int(k8[s:].abs().max()) == 0 if k8.shape[0] > s else True
        assert float(ks[:, nb:].abs().max()) == 0.0 if ks.shape[1] > nb else True
        rv8, rvs = so.quant_v(v, heads)
        pos = so.vt_position(s, device="cuda")
        vt8, vs = ops.sage_quant_vt(v, heads)
        got = vt8.reshape(heads, 128, -1)[:, :, pos].transpose(1, 2)               # [H, S, 128] codes
        assert torch.equal(got, rv8.view(torch.uint8)) and torch.equal(vs, rvs), ("v", s)
        pad = torch.ones(vt8.shape[1], dtype=torch.bool, device="cuda")
        pad[pos] = False
        assert int(vt8[:, pad].max()) == 0 if pad.any() else True


def _plain_from_vt32(vt, n, kv_len):
    """the V [kv_len, n] a gf_linear_vt32(_fp8) V^T holds: inside every 32-key group key 4 g + i sits at 8 g + i, key 16 + 4 g + i at 8 g + 4 + i"""
    kv_pad = -(-kv_len // 64) * 64
    key = torch.arange(kv_len, device=vt.device)
    w, g, i = key % 32, (key % 16) // 4, key % 4
    pos = key - w + 8 * g + i + 4 * (w >= 16).long()
    return vt[: n * kv_pad].view(n, kv_pad)[:, pos].t().contiguous()


def test_quant_vt_from_the_projection_layouts():
    """the bf16 V^T that gf_linear_vt32 / gf_linear_vt32_fp8 write (key lengths >= ops.VT_MIN_KV, the block path's condition) gives
    the e4m3 V^T and the attention output of the plain V it holds"""
    ops = _sage()
    heads = 5
    for s in (ops.VT_MIN_KV, 2113, 4097):
        assert ops.vt32_ok(s, heads, 128)
        x = torch.randn((s, 512), device="cuda").to(BF)
        w = (torch.randn((heads * 128, 512), device="cuda") * 0.05).to(BF)
        b = (torch.randn((heads * 128,), device="cuda") * 0.1).to(BF)
        q, k, _ = _qkv(s, s, heads, seed=s)
        x8, xs = ops.quant_fp8_rowscale(x)
        for vt in (ops.linear_vt32(x, w, b).clone(), ops.linear_vt32_fp8(x8, xs, ops.cast_fp8(w), b).clone()):   # bf16 / config 5
            v = _plain_from_vt32(vt, heads * 128, s)
            a8, asc = ops.sage_quant_vt(v, heads)
            b8, bsc = ops.sage_quant_vt(None, heads, vt=vt, kv_len=s)
            assert torch.equal(a8, b8) and torch.equal(asc, bsc), s
            assert torch.equal(ops.sage_attn(q, k, v, heads), ops.sage_attn(q, k, None, heads, vt=vt)), s


@pytest.mark.parametrize("heads", [1, 5, 40])
def test_attention_matches_oracle(heads):
    ops = _sage()
    shapes = SHAPES if heads < 40 else [1, 33, 65, 2047, 4097]
    for s in shapes:
        q, k, v = _qkv(s, s, heads, seed=100 + s)
        o = ops.sage_attn(q, k, v, heads)
        mu = ops.sage_k_mean(k, heads)
        ref = so.attention(q, k, v, heads, mu, T=ops.SAGE_T, tau=ops.SAGE_TAU, e=ops.SAGE_E)
        assert _rel(o, ref) <= BAR, (heads, s, _rel(o, ref))
    # cross lengths (q and keys differ)
    q, _, _ = _qkv(300, 300, heads, seed=7)
    _, k, v = _qkv(1000, 1000, heads, seed=8)
    mu = ops.sage_k_mean(k, heads)
    assert _rel(ops.sage_attn(q, k, v, heads), so.attention(q, k, v, heads, mu)) <= BAR


def test_attention_production_shape_sampled_rows():
    ops = _sage()
    s, heads = 32760, 40
    q, k, v = _qkv(s, s, heads, seed=5)
    o = ops.sage_attn(q, k, v, heads)
    mu = ops.sage_k_mean(k, heads)
    rows = torch.cat([torch.arange(0, 40), torch.randint(0, s, (88,), generator=torch.Generator().manual_seed(1)),
                      torch.arange(s - 40, s)]).cuda()
    ref = so.attention(q, k, v, heads, mu, rows=rows)
    assert _rel(o[rows], ref) <= BAR


@pytest.mark.parametrize("std", [1.0, 3.0, 8.0])
def test_peaky_logits_error_from_fp64_not_above_the_oracle(std):
    """logit std 1 / 3 / 8: the kernel's error from fp64 attention within 1.05 x the recipe's own"""
    ops = _sage()
    s, heads = 2048, 4
    g = torch.Generator(device="cuda").manual_seed(int(std))
    q = (torch.randn((s, heads * 128), generator=g, device="cuda") * math.sqrt(std)).to(BF)
    k = (torch.randn((s, heads * 128), generator=g, device="cuda") * math.sqrt(std)).to(BF)
    v = torch.randn((s, heads * 128), generator=g, device="cuda").to(BF)
    exact = so.attention_fp64(q, k, v, heads)
    mu = ops.sage_k_mean(k, heads)
    e_kernel = _rel(ops.sage_attn(q, k, v, heads), exact)
    e_oracle = _rel(so.attention(q, k, v, heads, mu), exact)
    hq, hk, hv = (t.reshape(s, heads, 128).transpose(0, 1)[None] for t in (q, k, v))
    sdpa = torch.nn.functional.scaled_dot_product_attention(hq, hk, hv)[0].transpose(0, 1).reshape(s, heads * 128)
    print(f"logit std {std:g}: sage kernel {e_kernel:.3e}, sage oracle {e_oracle:.3e}, kernel 3 "
          f"{_rel(ops.flash_attn(q, k, v, heads), exact):.3e}, torch SDPA {_rel(sdpa, exact):.3e}")
    assert e_kernel <= 1.05 * e_oracle, (e_kernel, e_oracle)


@pytest.mark.parametrize("ramp", [8.0, 40.0])
def test_adversarial_ramp_keeps_p_in_range(ramp):
    """DESIGN §5.3's worst case for a lazy rescale: logits rising by `ramp` log2 units per 64-key tile, all mass on the last keys"""
    ops = _sage()
    s, heads, hd = 4096, 2, 128
    tiles = s // 64
    amp = math.sqrt(ramp * tiles * math.log(2.0) * math.sqrt(hd))
    u = torch.ones((hd,), device="cuda") / math.sqrt(hd)
    q = (amp * u).repeat(heads)[None, :].expand(s, heads * hd).contiguous().to(BF)
    k = ((torch.arange(s, device="cuda", dtype=torch.float32) / s)[:, None] * (amp * u).repeat(heads)[None, :]).to(BF)
    v = torch.randn((s, heads * hd), device="cuda").to(BF)
    o = ops.sage_attn(q, k, v, heads)
    assert torch.isfinite(o.float()).all()
    mu = ops.sage_k_mean(k, heads)
    # every query row is the same here, so one P that the kernel's exp2 rounds across an e4m3 boundary the other way repeats in all of
    # them instead of averaging out: 6.3e-4 measured at r = 40; bar 1.5e-3, still 25 x below the recipe's error from fp64
    assert _rel(o, so.attention(q, k, v, heads, mu)) <= 1.5e-3


def _sage_self_attention(x, freqs, sd, pre, num_heads, eps):
    """oracle.wan_oracle.self_attention with the attention replaced by the sage oracle (cross-attention keeps the exact one)"""
    from oracle import wan_oracle as wo
    q = wo.rms_norm(wo._lin(x, sd, pre + "q"), sd[pre + "norm_q.weight"], eps)
    k = wo.rms_norm(wo._lin(x, sd, pre + "k"), sd[pre + "norm_k.weight"], eps)
    v = wo._lin(x, sd, pre + "v")
    q = wo.rope_apply(q, freqs, num_heads)
    k = wo.rope_apply(k, freqs, num_heads)
    outs = []
    for b in range(q.shape[0]):
        kb = k[b].to(BF)
        mu = kb.float().reshape(kb.shape[0], num_heads, 128).mean(0)
        outs.append(so.attention(q[b].to(BF), kb, v[b].to(BF), num_heads, mu).to(q.dtype))
    return wo._lin(torch.stack(outs), sd, pre + "o")


@pytest.mark.parametrize("fp8", [False, True])
def test_block_with_sage_attention_vs_oracle_block(fp8, monkeypatch):
    import torch.nn.functional as F
    from goal_force_amd.dit import DiTBlock, RopeTable, enable_fp8, enable_sage_attention, precompute_freqs_cis_3d
    from oracle import fp8_oracle as fo
    from oracle import wan_oracle as wo
    cfg = gi.TINY
    grid = (4, 8, 12)                                  # 384 tokens: 12 Q scale blocks, 6 K blocks, 3 key tiles
    n = grid[0] * grid[1] * grid[2]
    sd = gi.block_sd(torch.Generator().manual_seed(21), cfg["dim"], cfg["ffn_dim"], "", BF)
    x, ctx, t_mod = gi.block_inputs(cfg["dim"], n, gi.TINY_CTX_LEN, seed=22)
    freqs = wo.rope_freqs_3d(128, *grid)
    sd32 = {k_: v_.float() for k_, v_ in sd.items()}
    truth = wo.dit_block(x.float(), ctx.float(), t_mod.float(), freqs, sd32, "", cfg["num_heads"], cfg["eps"])
    sd_gpu = {k_: v_.cuda() for k_, v_ in sd.items()}
    wlin = {id(t) for k_, t in sd_gpu.items() if k_.endswith(".weight") and t.dim() == 2}
    if fp8:
        monkeypatch.setattr(wo, "LINEAR", lambda a, w, b=None: fo.fp8_linear(a, w, b) if id(w) in wlin else F.linear(a, w, b))
    monkeypatch.setattr(wo, "self_attention", _sage_self_attention)
    ref = wo.dit_block(x.cuda(), ctx.cuda(), t_mod.cuda(), freqs.cuda(), sd_gpu, "", cfg["num_heads"],
                       cfg["eps"]).cpu()
    blk = DiTBlock(False, cfg["dim"], cfg["num_heads"], cfg["ffn_dim"], cfg["eps"])
    blk.load_state_dict(sd, strict=True)
    blk = blk.to(BF).cuda()
    if fp8:
        enable_fp8(blk)
    rope = RopeTable.from_grid(precompute_freqs_cis_3d(128), *grid, "cuda")
    torch.set_grad_enabled(False)
    plain = blk(x.cuda(), ctx.cuda(), t_mod.cuda(), rope).cpu()
    enable_sage_attention(blk)
    got = blk(x.cuda(), ctx.cuda(), t_mod.cuda(), rope).cpu()
    enable_sage_attention(blk, False)
    back = blk(x.cuda(), ctx.cuda(), t_mod.cuda(), rope).cpu()
    assert torch.equal(back, plain), "switching off must give the bits of the never-switched module"
    assert not torch.equal(got, plain)
    e_got, e_ref = _rel(got.float(), truth), _rel(ref.float(), truth)
    print(f"fp8={fp8}: sage block {e_got:.3e} from fp32, oracle sage block {e_ref:.3e}, flash block {_rel(plain.float(), truth):.3e}")
    assert e_got <= 1.25 * e_ref, (e_got, e_ref)


def test_sageattn_drop_in():
    from einops import rearrange
    from goal_force_amd import dit
    ops = _sage()
    heads, s = 3, 300
    q, k, v = (t.unsqueeze(0) for t in _qkv(s, s, heads, seed=11))
    want = ops.sage_attn(q[0], k[0], v[0], heads)
    hq, hk, hv = (rearrange(t, "b s (n d) -> b n s d", n=heads) for t in (q, k, v))   # DIT:50-54's strided views
    got = dit.sageattn(hq, hk, hv)
    assert torch.equal(rearrange(got, "b n s d -> b s (n d)")[0], want)
    nq, nk, nv = (t.reshape(1, s, heads, 128) for t in (q, k, v))
    assert torch.equal(dit.sageattn(nq, nk, nv, tensor_layout="NHD").reshape(s, heads * 128), want)
    sc = 0.05
    assert torch.equal(dit.sageattn(hq, hk, hv, sm_scale=sc).transpose(1, 2).reshape(s, heads * 128),
                       ops.sage_attn(q[0], k[0], v[0], heads, scale=sc))
    assert not torch.equal(ops.sage_attn(q[0], k[0], v[0], heads, scale=sc), want)


def _free_port():
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    p = sk.getsockname()[1]
    sk.close()
    return p


def _sp_forward(sp):
    from goal_force_amd.controlnet import ControlNet
    from goal_force_amd.dit import WanModel, enable_sage_attention
    from goal_force_amd.model_fn import model_fn_wan_video
    torch.set_grad_enabled(False)
    cfg = gi.TINY
    dit = WanModel(has_image_input=False, require_clip_embedding=False, **cfg)
    dit.load_state_dict(gi.dit_sd(cfg, seed=41), strict=True)
    cn = ControlNet(gi.TINY_CONTROLNET_LAYERS, dim=cfg["dim"], num_heads=cfg["num_heads"], ffn_dim=cfg["ffn_dim"])
    cn.load_state_dict(gi.controlnet_sd(cfg, gi.TINY_CONTROLNET_LAYERS, seed=42, zero_convs_zero=False), strict=True)
    dit, cn = dit.to(BF).cuda(), cn.to(BF).cuda()
    enable_sage_attention(dit)
    enable_sage_attention(cn)
    inp = {k_: v_.cuda() for k_, v_ in gi.tiny_inputs().items()}
    ts = torch.tensor([995.9], dtype=BF).cuda()
    return model_fn_wan_video(dit, latents=inp["latents"], timestep=ts, context=inp["ctx_posi"], y=inp["y"], controlnet=cn,
                              control_signal_video_latents=inp["control"], elide_zero_controlnet=False, sequence_parallel=sp).cpu()


def _sp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    sys.path.insert(0, os.path.dirname(__file__))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from goal_force_amd.sequence_parallel import SequenceParallel
        torch.save(_sp_forward(SequenceParallel()), os.path.join(out, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_head_parallel_sage_is_bit_identical(tmp_path):
    """P = 2 head-parallel with the switch on: every quantisation is per head, so the sharded forward is the one-GPU forward bit for bit"""
    world = 2
    mp.spawn(_sp_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    want = _sp_forward(None)
    for r in range(world):
        assert torch.equal(torch.load(os.path.join(tmp_path, f"r{r}.pt")), want), r


def test_training_refuses_a_switched_module():
    from goal_force_amd import training
    from goal_force_amd._lib import GoalForceError
    from goal_force_amd.dit import DiTBlock, RopeTable, enable_sage_attention, precompute_freqs_cis_3d
    cfg = gi.TINY
    blk = DiTBlock(False, cfg["dim"], cfg["num_heads"], cfg["ffn_dim"], cfg["eps"])
    blk.load_state_dict(gi.block_sd(torch.Generator().manual_seed(11), cfg["dim"], cfg["ffn_dim"], "", BF), strict=True)
    blk = blk.to(BF).cuda()
    enable_sage_attention(blk)
    x, ctx, t_mod = gi.block_inputs(cfg["dim"], 72, gi.TINY_CTX_LEN, seed=12)
    rope = RopeTable.from_grid(precompute_freqs_cis_3d(128), 3, 4, 6, "cuda")
    with pytest.raises(GoalForceError, match="enable_sage_attention"):
        training.block_forward(blk, x[0].cuda().requires_grad_(True), ctx[0].cuda(), t_mod.cuda(), rope)
