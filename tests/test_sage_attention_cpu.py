"""SageAttention backend, host side: the oracle's self-checks (tests/sage_oracle.py), the C ABI's declarations and exports, and the
refusals that need no GPU."""
import os
import re

import pytest
import torch

import sage_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAGE_SYMBOLS = ("gf_sage_workspace_bytes", "gf_sage_k_mean", "gf_sage_quant_q", "gf_sage_quant_k", "gf_sage_quant_vt", "gf_sage_attn_fwd",
                "gf_sage_attn")


def _qkv(sq, skv, heads, seed=0, std=1.0):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn((sq, heads * 128), generator=g) * std).to(torch.bfloat16)
    k = (torch.randn((skv, heads * 128), generator=g) + 0.5 * torch.randn((1, heads * 128), generator=g)).to(torch.bfloat16)
    v = torch.randn((skv, heads * 128), generator=g).to(torch.bfloat16)
    return q, k, v


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("skv", [1, 63, 128, 200, 257])
def test_oracle_without_quantisation_is_exact_attention(skv):
    """quantize=False keeps the tiles, the smoothing and the online softmax but no rounding: it must be the fp64 attention, ragged
    tails included."""
    q, k, v = _qkv(37, skv, 2, seed=skv)
    mu = k.float().reshape(skv, 2, 128).mean(0)
    o = so.attention(q, k, v, 2, mu, quantize=False)
    assert _rel(o, so.attention_fp64(q, k, v, 2)) < 1e-12


def test_smoothing_alone_changes_nothing():
    q, k, v = _qkv(40, 300, 2, seed=3)
    mu = torch.randn((2, 128), generator=torch.Generator().manual_seed(9)) * 3
    a = so.attention(q, k, v, 2, mu, quantize=False)
    b = so.attention(q, k, v, 2, torch.zeros((2, 128)), quantize=False)
    assert _rel(a, b) < 1e-12


def test_int8_blocks_hand_built():
    x = torch.zeros((1, 96, 128))
    x[0, 0, 0] = -2.0                    # block 0: amax 2 at a negative entry -> code -127
    x[0, 1, 5] = 1.0                     # 1 * 127 / 2 = 63.5 -> 64 (tie to even)
    x[0, 2, 7] = 2.0 * 62.5 / 127        # -> about 62.5
    x[0, 40, 3] = 0.25                   # block 1: amax 0.25 -> code 127
                                         # block 2 (rows 64 .. 95) all zero
    codes, scale = so.quant_int8(x, 32)
    f32 = lambda a, b: float(torch.tensor(a) / torch.tensor(b))          # noqa: E731 — fp32 division
    assert scale[0].tolist() == [f32(2.0, 127.0), f32(0.25, 127.0), 0.0]
    assert codes[0, 0, 0] == -127 and codes[0, 1, 5] == 64 and codes[0, 40, 3] == 127
    assert codes[0, 2, 7] == round(float(torch.tensor(2.0 * 62.5 / 127) * (torch.tensor(127.0) / torch.tensor(2.0))))
    assert int(codes[0, 64:].abs().max()) == 0 and int(codes.abs().max()) == 127
    # ties: a value whose fp32 product is exactly k + 0.5 rounds to the even neighbour
    y = torch.zeros((1, 32, 128))
    y[0, 0, 0] = 127.0
    y[0, 0, 1:6] = torch.tensor([0.5, 1.5, 2.5, -0.5, -2.5])
    c, s = so.quant_int8(y, 32)
    assert float(s[0, 0]) == 1.0 and c[0, 0, :6].tolist() == [127, 0, 2, 2, 0, -2]


def test_e4m3_value_scales():
    v = torch.zeros((5, 128), dtype=torch.bfloat16)
    v[0, 0], v[3, 0], v[2, 1] = 3.0, -6.0, 0.5
    codes, scale = so.quant_v(v, 1)
    assert float(scale[0, 0]) == float(torch.tensor(6.0) / torch.tensor(448.0)) and float(scale[0, 2]) == 0.0
    assert float(codes[0, 3, 0].float()) == -448.0 and float(codes[0, 0, 0].float()) == 224.0
    assert float(codes[0, 2, 1].float()) == 448.0 and float(codes[0, :, 2].float().abs().max()) == 0.0


def test_quantised_oracle_is_close_to_fp64_on_ragged_tails():
    """the recipe's own error from fp64 (a few 1e-2 at logit std 1, set by the e4m3 V): finite, small, and tile-size independent in order of magnitude"""
    q, k, v = _qkv(65, 333, 2, seed=5)
    mu = k.float().reshape(333, 2, 128).mean(0)
    ref = so.attention_fp64(q, k, v, 2)
    for T in (64, 128):
        e = _rel(so.attention(q, k, v, 2, mu, T=T), ref)
        assert 1e-3 < e < 6e-2, (T, e)          # e4m3 V (3 mantissa bits) dominates: ~3.6e-2


def test_vt_positions_are_a_permutation_of_every_slice():
    pos = so.vt_position(384)
    assert sorted(pos.tolist()) == list(range(384))
    assert pos[:8].tolist() == [0, 1, 2, 3, 32, 33, 34, 35] and pos[16].item() == 4


def test_header_declares_and_library_exports_the_sage_entry_points():
    hdr = open(os.path.join(ROOT, "include", "goalforce.h")).read()
    for s in SAGE_SYMBOLS:
        assert re.search(r"GF_API\s+[\w\s\*]+\b" + s + r"\(", hdr), s
    from goal_force_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 20 and lib.gf_abi_version() == 20
    for s in SAGE_SYMBOLS:
        assert s in _lib.SYMBOLS and hasattr(lib, s), s
    # the workspace query is host arithmetic: no device needed
    assert lib.gf_sage_workspace_bytes(32760, 32760, 40) > 3 * 32760 * 40 * 128
    assert lib.gf_sage_workspace_bytes(1, 0, 1) == 0


def test_refusals_without_a_gpu():
    from goal_force_amd import dit, ops
    from goal_force_amd._lib import GoalForceError
    q = torch.zeros((1, 2, 64, 128), dtype=torch.bfloat16)
    with pytest.raises(GoalForceError, match="is_causal"):
        dit.sageattn(q, q, q, is_causal=True)
    with pytest.raises(GoalForceError, match="return_lse"):
        dit.sageattn(q, q, q, return_lse=True)
    with pytest.raises(GoalForceError, match="head_dim 64"):
        dit.sageattn(q[..., :64], q[..., :64], q[..., :64])
    with pytest.raises(GoalForceError, match="tensor_layout"):
        dit.sageattn(q, q, q, tensor_layout="BHSD")
    with pytest.raises(GoalForceError, match="GPU"):
        ops.sage_attn(q[0, 0], q[0, 0], q[0, 0], 1)
    for bad in (-0.1, 0.0, float("inf"), float("nan")):
        with pytest.raises(GoalForceError, match="scale"):
            dit.sageattn(q, q, q, sm_scale=bad)
    from goal_force_amd.sequence_parallel import _backend
    with pytest.raises(GoalForceError, match="backend"):
        _backend("sdpa")


def test_training_refuses_a_switched_block():
    from goal_force_amd import dit, training
    from goal_force_amd._lib import GoalForceError
    blk = dit.DiTBlock(False, 256, 2, 512)
    dit.enable_sage_attention(blk)
    x = torch.zeros((72, 256), dtype=torch.bfloat16)
    with pytest.raises(GoalForceError, match="enable_sage_attention"):
        training.block_forward(blk, x, torch.zeros((8, 256), dtype=torch.bfloat16), torch.zeros((1, 6, 256), dtype=torch.bfloat16), None)
    with pytest.raises(GoalForceError, match="enable_sage_attention"):
        blk.self_attn.attend(x, None, keep={})
    dit.enable_sage_attention(blk, False)
    assert not blk.self_attn._gf_sage
