"""The fused MXFP4 producers without a GPU: the declarations of gf_layernorm_modulate_mxfp4 and gf_gemm_mxfp4_q4, their ctypes forms,
the unchanged ABI revision, the `fp4_fused` option and the refusals of ops.gemm_mxfp4_q4 that need no device.
"""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8 = torch.uint8


def test_header_declares_the_two_entry_points_and_the_bindings_have_them():
    from goal_force_amd import _lib
    text = " ".join(open(os.path.join(ROOT, "include", "goalforce.h"), encoding="utf-8").read().split())
    ln = ("GF_API int gf_layernorm_modulate_mxfp4(const void* x, void* out4, void* scales, const void* weight, const void* bias, "
          "const void* scale1p, const void* shift, int64_t rows, int64_t dim, int64_t x_stride, int64_t out_stride, int64_t scale_stride, "
          "float eps, void* stream);")
    q4 = ("GF_API int gf_gemm_mxfp4_q4(const void* A4, int64_t lda, const void* a_scale, int64_t a_scale_stride, const void* W4, int64_t ldw, "
          "const void* w_scale, int64_t w_scale_stride, const void* bias, void* C4, int64_t ldc4, void* c_scale, int64_t c_scale_stride, "
          "int64_t M, int64_t N, int64_t K, int epilogue, void* stream);")
    assert ln in text and q4 in text
    import ctypes
    p, i64, i, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    assert _lib.BINDINGS["gf_layernorm_modulate_mxfp4"] == (i, [p, p, p, p, p, p, p, i64, i64, i64, i64, i64, f, p])
    assert _lib.BINDINGS["gf_gemm_mxfp4_q4"] == (i, [p, i64, p, i64, p, i64, p, i64, p, p, i64, p, i64, i64, i64, i64, i, p])
    assert _lib.ABI_VERSION == 20 and re.search(r"^#define GF_ABI_VERSION 20\s*$", open(_lib.HEADER_PATH).read(), flags=re.M)


def test_the_block_quantiser_is_stated_once():
    """e2m1_code and the block step live in one header; the three users include it and none restates the recipe."""
    csrc = os.path.join(ROOT, "goal_force_amd", "csrc")
    texts = {n: open(os.path.join(csrc, n), encoding="utf-8").read() for n in os.listdir(csrc) if n.endswith((".hip", ".h", ".inc"))}
    assert [n for n, t in texts.items() if re.search(r"unsigned e2m1_code\(", t)] == ["gf_mxfp4_quant.h"]
    assert [n for n, t in texts.items() if re.search(r"unsigned mxfp4_block_step\(", t)] == ["gf_mxfp4_quant.h"]
    for user in ("gf_gemm_mxfp4.hip", "gf_rowops.hip"):
        assert '#include "gf_mxfp4_quant.h"' in texts[user] and "mxfp4_block_step(" in texts[user]


def test_fp4_fused_option_defaults_on_and_round_trips():
    from goal_force_amd import ops
    from goal_force_amd._lib import GoalForceError
    assert ops.option("fp4_fused") is True
    with ops.options(fp4_fused=False):
        assert ops.option("fp4_fused") is False
        with ops.options(fp4_fused=1):
            assert ops.option("fp4_fused") is True
        assert ops.option("fp4_fused") is False
    assert ops.option("fp4_fused") is True
    with pytest.raises(GoalForceError, match="unknown option"):
        ops.options(fp4_fuse=False)


def test_the_wrappers_exist_and_refuse_what_needs_no_device():
    from goal_force_amd import ops
    from goal_force_amd._lib import GoalForceError
    assert callable(ops.layernorm_modulate_mxfp4) and callable(ops.gemm_mxfp4_q4)
    M, K = 4, 256
    a4, sa = torch.zeros((M, K // 2), dtype=U8), torch.zeros((M, K // 32), dtype=U8)
    for N in (40, 8, 264):
        w4, sw = torch.zeros((N, K // 2), dtype=U8), torch.zeros((N, K // 32), dtype=U8)
        with pytest.raises(GoalForceError, match=rf"gemm_mxfp4_q4: N = {N} output features must be a multiple of 32"):
            ops.gemm_mxfp4_q4(a4, sa, w4, sw)
    w4, sw = torch.zeros((64, K // 2), dtype=U8), torch.zeros((64, K // 32), dtype=U8)
    for epi in (ops.EPI_BIAS_GATE_RESID, ops.EPI_BIAS_RESID, ops.EPI_BIAS_MUL, 6, -1):
        with pytest.raises(GoalForceError, match=rf"gemm_mxfp4_q4: epilogue {epi} is not one of EPI_BIAS, EPI_BIAS_GELU_TANH, EPI_BIAS_SILU"):
            ops.gemm_mxfp4_q4(a4, sa, w4, sw, epilogue=epi)
    # a legal shape and epilogue reaches the operand checks: no CPU fallback exists
    with pytest.raises(GoalForceError, match="must be on the GPU"):
        ops.gemm_mxfp4_q4(a4, sa, w4, sw, epilogue=ops.EPI_BIAS_GELU_TANH)
    with pytest.raises(GoalForceError, match="must be on the GPU"):
        ops.layernorm_modulate_mxfp4(torch.zeros((2, 1536), dtype=torch.bfloat16))
