"""The cross-attention's output projection folded into the cached values: gf_cross_probs (normalised probabilities
instead of the attention output), gf_cross_fold_table (U = V_h W_o,h^T) and the dispatch in dit.DiTBlock / model_fn."""
import math

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from goal_force_amd import ops as _ops
    return _ops


def _probs_fp64(q, k, heads, m):
    """softmax over [k_0 .. k_{n-2}, k_{n-1} x m] in fp64 -> [Sq, heads, n] (the last column: the m copies' total)."""
    sq, n = q.shape[0], k.shape[0]
    qd = q.double().view(sq, heads, 128).transpose(0, 1)
    kd = k.double().view(n, heads, 128).transpose(0, 1)
    s = qd @ kd.transpose(1, 2) / math.sqrt(128)
    s[:, :, n - 1] += math.log(m)
    return torch.softmax(s, -1).transpose(0, 1)


@pytest.mark.parametrize("n_keys", [1, 17, 41, 63])
@pytest.mark.parametrize("m", [1, 472])
def test_cross_probs_vs_fp64_softmax(ops, n_keys, m):
    """Every probability within one bf16 rounding (plus fp32 score noise) of the fp64 softmax; the last key's weight plus its residue
    column within fp32 noise; the columns after it exactly zero; a ragged query block (300 rows) and logits of std 3.  n_keys 63: the
    residue in the tile's last column (n_pad 64)."""
    g = torch.Generator().manual_seed(n_keys * 1000 + m)
    heads, sq = 3, 300
    q = (torch.randn(sq, heads * 128, generator=g) * 3).to(BF)
    k = torch.randn(n_keys, heads * 128, generator=g).to(BF)
    n_pad = -(-(n_keys + 1) // 16) * 16
    got = ops.cross_probs(q.cuda(), k.cuda(), heads, n_pad, last_key_mult=m).cpu().view(sq, heads, n_pad)
    ref = _probs_fp64(q, k, heads, m)
    assert torch.equal(got[:, :, n_keys + 1:], torch.zeros_like(got[:, :, n_keys + 1:]))
    err = (got[:, :, :n_keys].double() - ref).abs()
    assert bool((err <= ref * (2.0 ** -8 + 1e-4) + 1e-7).all()), float((err / ref.clamp_min(1e-30)).max())
    last = got[:, :, n_keys - 1].double() + got[:, :, n_keys].double()
    assert bool(((last - ref[:, :, -1]).abs() <= ref[:, :, -1] * 2e-4 + 1e-7).all())
    assert float((got.double().sum(-1) - 1).abs().max()) < 2e-2


def _module(dim, heads, seed, q_gain):
    from goal_force_amd import dit
    g = torch.Generator().manual_seed(seed)
    ca = dit.CrossAttention(dim, heads).to(BF).cuda()
    for p_ in ca.parameters():
        p_.data.copy_((torch.randn(p_.shape, generator=g) * (1.0 / math.sqrt(dim) if p_.dim() == 2 else 0.02)).to(BF))
    ca.norm_q.weight.data.fill_(q_gain)       # logit std ~ q_gain (q and k leave their RMSNorm at unit RMS)
    ca.norm_k.weight.data.fill_(1.0)
    return ca, g


@pytest.mark.parametrize("logit_std", [1.0, 3.0, 8.0])
def test_folded_projection_vs_fp64(ops, logit_std):
    """The cross-attention module's output (q / k / v projections, norms, attention, o projection) on a 40-token prompt padded to 512,
    folded (probabilities @ U^T) and unfolded (attention, then W_o), against the module evaluated in fp64 on the same inputs and
    weights, rel-L2 as tools/fuzz_ops.py measures it: the folded path is within 1.1 x the unfolded one and within 1.1 x the
    reference's own bf16 chain (oracle.wan_oracle.cross_attention on bf16 tensors: torch SDPA over all 512 keys).  Measured:
    0.98-1.01 x the unfolded path, 0.86-1.01 x the reference chain."""
    from goal_force_amd import dit
    from oracle import wan_oracle as wo
    torch.set_grad_enabled(False)
    dim, heads, sq = 1024, 8, 700
    ca, g = _module(dim, heads, int(logit_std * 10), logit_std)
    h = torch.randn(sq, dim, generator=g).to(BF).cuda()
    ctx = torch.randn(512, dim, generator=g).to(BF)
    ctx[40:] = ctx[40:41]                                    # the prompter's padding: rows 40 .. 511 identical (41 keys, the last x 472)
    ctx = ctx.cuda()
    kv = ca.context_kv(ctx)
    assert kv[2] == 472 and ca.fold_ok(kv)
    folded = ops.gemm(ca.attend_probs(h, kv), ca.fold_table(kv), ca.o.bias)
    plain = dit.linear(ca.attend(h, kv), ca.o)
    sd = ca.state_dict()
    ref = wo.cross_attention(h.double()[None], ctx.double()[None], {n: t.double() for n, t in sd.items()}, "", heads, ca.norm_q.eps)[0]
    chain = wo.cross_attention(h[None], ctx[None], sd, "", heads, ca.norm_q.eps)[0]
    e_fold, e_plain, e_ref = rel_l2(folded, ref), rel_l2(plain, ref), rel_l2(chain, ref)
    print(f"logit std {logit_std}: folded {e_fold:.3e}, unfolded {e_plain:.3e}, reference bf16 chain {e_ref:.3e}")
    assert e_fold <= 1.1 * e_plain and e_fold <= 1.1 * e_ref, (e_fold, e_plain, e_ref)


def test_zero_pad_columns_contribute_nothing(ops):
    """P^ and U are written with exact zeros in the columns n_keys + 1 .. n_pad - 1 of every head (column n_keys: the last key's
    residue and its copy of U): whatever the other operand holds there, the projection GEMM returns the same bits."""
    torch.set_grad_enabled(False)
    ca, g = _module(512, 4, 3, 1.0)
    ctx = torch.randn(512, 512, generator=g).to(BF)
    ctx[20:] = ctx[20:21]                                    # 21 keys (+ the residue column) -> n_pad 32
    kv = ca.context_kv(ctx.cuda())
    h = torch.randn(333, 512, generator=g).to(BF).cuda()
    p, u = ca.attend_probs(h, kv), ca.fold_table(kv)
    pad = torch.zeros(4, 32, dtype=torch.bool)
    pad[:, 22:] = True
    pad = pad.flatten().cuda()
    assert p.shape == (333, 128) and u.shape == (512, 128)
    assert not bool(p[:, pad].any()) and not bool(u[:, pad].any())
    base = ops.gemm(p, u, ca.o.bias)
    u_junk, p_junk = u.clone(), p.clone()
    u_junk[:, pad] = torch.randn(512, int(pad.sum()), generator=g).to(BF).cuda()
    p_junk[:, pad] = torch.randn(333, int(pad.sum()), generator=g).to(BF).cuda()
    assert torch.equal(ops.gemm(p, u_junk, ca.o.bias), base)
    assert torch.equal(ops.gemm(p_junk, u, ca.o.bias), base)
    # U's live columns are V_h W_o,h^T rounded once
    k, v, _ = kv
    ref = torch.einsum("jhd,nhd->nhj", v.double().view(21, 4, 128), ca.o.weight.double().view(512, 4, 128))
    got = u.view(512, 4, 32)[:, :, :21].double()
    assert bool(((got - ref).abs() <= ref.abs() * 2.0 ** -8 + 1e-6).all())
    assert torch.equal(u.view(512, 4, 32)[:, :, 21], u.view(512, 4, 32)[:, :, 20])


def test_dispatch_falls_back(ops):
    """The folded path only serves an inference forward over pad-folded keys with a bf16 o projection: 512 distinct keys,
    fold_pad_keys=False, the fp8_linear contract, autograd (the training forward) and ops.options(fold_cross_o=False) keep the
    unfolded path — and a DiTBlock forward on the folded path stays within bf16 rounding of the unfolded one."""
    from goal_force_amd import dit
    torch.set_grad_enabled(False)
    g = torch.Generator().manual_seed(11)
    blk = dit.DiTBlock(False, 256, 2, 512).to(BF).cuda()
    for p_ in blk.parameters():
        p_.data.copy_((torch.randn(p_.shape, generator=g) * (0.06 if p_.dim() == 2 else 0.02)).to(BF))
    ctx = torch.randn(1, 512, 256, generator=g).to(BF)
    ctx[:, 30:] = ctx[:, 30:31]
    ctx = ctx.cuda()
    ca = blk.cross_attn
    kv = ca.context_kv(ctx[0])
    assert kv[2] == 482 and ca.fold_ok(kv)
    assert not ca.fold_ok(ca.context_kv(torch.randn(512, 256, generator=g).to(BF).cuda()))          # 512 distinct keys
    with ops.options(fold_pad_keys=False):
        assert not ca.fold_ok(ca.context_kv(ctx[0]))
    with ops.options(fold_cross_o=False):
        assert not ca.fold_ok(kv)
    assert ca.fold_ok(kv), "the option is restored on leaving the block"
    with torch.enable_grad():
        assert not ca.fold_ok(kv)
    x = torch.randn(1, 100, 256, generator=g).to(BF).cuda()
    t_mod = (torch.randn(1, 6, 256, generator=g) * 0.5).to(BF).cuda()
    rope = dit.RopeTable(dit.precompute_freqs_cis(128, 100), "cuda")
    calls = []
    real = ops.cross_probs
    ops.cross_probs = lambda *a, **kw: calls.append(1) or real(*a, **kw)
    try:
        folded = blk(x, ctx, t_mod, rope)
        assert len(calls) == 1
        with ops.options(fold_cross_o=False):
            plain = blk(x, ctx, t_mod, rope)
        assert len(calls) == 1
        blk(x, ctx, t_mod, rope, keep={})                     # the training forward (keeps tensors for the backward)
        assert len(calls) == 1
        dit.enable_fp8(blk)
        assert not ca.fold_ok(kv)
        blk(x, ctx, t_mod, rope)
        assert len(calls) == 1
    finally:
        ops.cross_probs = real
        dit.enable_fp8(blk, False)
    assert rel_l2(folded.float(), plain.float()) < 6e-3
