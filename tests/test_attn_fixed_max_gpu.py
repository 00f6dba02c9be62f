"""Kernel 3 with the softmax maximum fixed at the first tile's row maximum, and its repair launch (gf_flash_attn_fwd_vt32_fm /
_sparse_fm, the default of ops.flash_attn / flash_attn_lse / flash_attn_sparse at key lengths >= VT_MIN_KV).  The inputs are those
of attn_fixed_max_cases.py, which test_attn_fixed_max_cpu.py models on the CPU: q pre-scaled as dit.SelfAttention produces it.
Bars: 4e-3 rel-L2 against fp64 on random data and 5e-3 (8e-3 on the row a case is built around) on constructed inputs — those of
test_flash_attn_kernel3_vs_fp64 and test_flash_attn_kernel3_running_maximum_paths; the log-sum-exp bar is
test_flash_attn_lse_same_on_both_v_paths' 2e-2, the backward bar test_flash_attn_backward's 1e-2."""
import pytest
import torch

import attn_fixed_max_cases as fc
import sparse_refs as sr
from conftest import rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from goal_force_amd import ops as _ops
    assert _ops.lib_option("attn_fixed_max") == 1, "the fixed-maximum path is the default"
    return _ops


def _run(ops, q, k, v, heads, fixed=True):
    """(out CPU, flags CPU or None) of ops.flash_attn on the pre-scaled q."""
    with ops.options(attn_fixed_max=int(fixed)):
        out = ops.flash_attn(q.cuda(), k.cuda(), v.cuda(), heads, scale=fc.SCALE)
        flags = ops.last_attn_flags
    assert (flags is not None) == fixed
    return out.cpu(), (flags.cpu() if fixed else None)


@pytest.mark.parametrize("name,sq,skv,heads,std", fc.RANDOM)
def test_random_data_vs_fp64_and_no_repair(ops, name, sq, skv, heads, std):
    q, k, v = fc.random_case(1000 + int(std), sq, skv, heads, std)
    ref = fc.reference(q, k, v, heads)[0]
    got, flags = _run(ops, q, k, v, heads)
    exact, _ = _run(ops, q, k, v, heads, fixed=False)
    e, e_exact = rel_l2(got, ref), rel_l2(exact, ref)
    print(f"fixed-max accuracy {name} ({sq} x {skv}, {heads} heads): fixed {e:.3e}  exact {e_exact:.3e}  ratio {e / e_exact:.3f}")
    assert tuple(flags.shape) == (heads, -(-sq // 256), 8) and int(flags.count_nonzero()) == 0
    assert bool(torch.isfinite(got.float()).all()) and e < 4e-3 and e_exact < 4e-3


@pytest.mark.parametrize("name,key,rise", fc.RISES)
def test_large_rise_without_repair(ops, name, key, rise):
    q, k, v, real = fc.rise_case(key, rise)
    ref = fc.reference(q, k, v, fc.RISE_SHAPE[2])[0]
    got, flags = _run(ops, q, k, v, fc.RISE_SHAPE[2])
    cols = slice(128 * fc.RISE_HEAD, 128 * fc.RISE_HEAD + 128)
    e, e_row = rel_l2(got, ref), rel_l2(got[fc.RISE_ROW, cols], ref[fc.RISE_ROW, cols])
    print(f"fixed-max rise {name} (+{real:.1f} log2 units): {e:.3e}, row {e_row:.3e}")
    assert int(flags.count_nonzero()) == 0 and bool(torch.isfinite(got.float()).all())
    assert e < 5e-3 and e_row < 8e-3


def test_overflow_is_flagged_and_repaired_on_the_exact_path(ops):
    """One key 135 log2 units above the first tile for ONE query (row 270 of head 1: query block 1, wave 0).  Only that (head,
    query block) is flagged; its 44 rows are the exact path's bits; every other row is what the fixed-maximum launch wrote — the
    bits of a run whose row 270 is an ordinary row (no overflow, nothing repaired, every other input the same)."""
    sq, skv, heads = fc.RISE_SHAPE
    q, k, v, real = fc.rise_case(1000, fc.OVERFLOW_RISE)
    assert real >= 130
    ref = fc.reference(q, k, v, heads)[0]
    got, flags = _run(ops, q, k, v, heads)
    exact, _ = _run(ops, q, k, v, heads, fixed=False)
    want_flags = torch.zeros_like(flags)
    want_flags[fc.RISE_HEAD, fc.RISE_ROW // 256, (fc.RISE_ROW % 256) // 32] = 1
    assert torch.equal(flags, want_flags), flags.tolist()
    rows, cols = slice(256, sq), slice(128 * fc.RISE_HEAD, 128 * fc.RISE_HEAD + 128)
    assert torch.equal(got[rows, cols], exact[rows, cols])
    q2 = q.clone()
    fc.head(q2, fc.RISE_HEAD)[fc.RISE_ROW] = fc.head(q, fc.RISE_HEAD)[fc.RISE_ROW - 1]      # (head 1's columns alone: the row's other head stays)
    plain, flags2 = _run(ops, q2, k, v, heads)
    assert int(flags2.count_nonzero()) == 0
    keep = torch.ones((sq, heads * 128), dtype=torch.bool)
    keep[rows, cols] = False
    assert torch.equal(got[keep], plain[keep])
    e, e_row = rel_l2(got, ref), rel_l2(got[fc.RISE_ROW, cols], ref[fc.RISE_ROW, cols])
    assert bool(torch.isfinite(got.float()).all()) and e < 5e-3 and e_row < 8e-3


@pytest.mark.parametrize("case", ["negative_start", "all_equal", "huge_then_small"])
def test_edges(ops, case):
    q, k, v = getattr(fc, case + "_case")()
    ref = fc.reference(q, k, v, 2)[0]
    got, flags = _run(ops, q, k, v, 2)
    assert int(flags.count_nonzero()) == 0 and bool(torch.isfinite(got.float()).all())
    assert rel_l2(got, ref) < 5e-3 and rel_l2(got[7], ref[7]) < 8e-3, case


def test_lse_and_the_backward_fed_with_it(ops):
    """flash_attn_lse on the fixed-maximum path: lse = m0 + log2(l) against fp64 and against the exact path's; at 2048 keys the
    backward kernels rebuild P from it and meet test_flash_attn_backward's bar against fp32 autograd."""
    from test_training_gpu import _ref_attention_grads
    for sq, skv, heads in ((300, 2100, 3), (257, 2048, 2)):
        g = torch.Generator().manual_seed(sq + skv)
        q, k, v, dout = (torch.randn((n, heads * 128), generator=g).to(BF).cuda() for n in (sq, skv, skv, sq))
        o, lse = ops.flash_attn_lse(q, k, v, heads)
        assert ops.last_attn_flags is not None and int(ops.last_attn_flags.count_nonzero()) == 0
        with ops.options(attn_fixed_max=0):
            o_x, lse_x = ops.flash_attn_lse(q, k, v, heads)
        with torch.enable_grad():
            o_ref, lse_ref, dq_ref, dk_ref, dv_ref = _ref_attention_grads(q, k, v, dout, heads)
        e_lse, d_lse = float((lse.cpu() - lse_ref).abs().max()), float((lse - lse_x).abs().max())
        print(f"fixed-max lse {sq} x {skv}: vs fp32 {e_lse:.3e} (exact path {float((lse_x.cpu() - lse_ref).abs().max()):.3e}), vs exact {d_lse:.3e}")
        assert e_lse < 2e-2 and d_lse < 2e-2 and rel_l2(o.float().cpu(), o_ref) < 4e-3
        if skv == 2048:
            for name, a, r in zip(("dq", "dk", "dv"), ops.flash_attn_bwd(q, k, v, o, dout, lse, heads), (dq_ref, dk_ref, dv_ref)):
                e = rel_l2(a.float().cpu(), r)
                assert e < 1e-2, f"{name}: rel_l2={e:.3e}"


def test_sparse_full_map_window_map_and_repair(ops):
    sq, skv, heads = fc.RISE_SHAPE
    nt = -(-skv // 64)
    q, k, v, _ = fc.rise_case(1000, 60.0)
    dq, dk, dv = q.cuda(), k.cuda(), v.cuda()
    dense = ops.flash_attn(dq, dk, dv, heads, scale=fc.SCALE)
    full = ops.flash_attn_sparse(dq, dk, dv, heads, ops.BlockMap(torch.ones((2, nt), dtype=torch.bool), device="cuda"), scale=fc.SCALE)
    assert ops.last_attn_flags is not None and torch.equal(full, dense)
    # a window: query block b sees tiles 8 b .. 8 b + 19 and the ragged last tile; tile 15 (key 1000) is inside both rows
    mask = torch.zeros((2, nt), dtype=torch.bool)
    for b in range(2):
        mask[b, 8 * b:8 * b + 20] = True
        mask[b, nt - 1] = True
    bm = ops.BlockMap(mask, device="cuda")
    got, lse = ops.flash_attn_sparse(dq, dk, dv, heads, bm, scale=fc.SCALE, lse=True)
    assert int(ops.last_attn_flags.count_nonzero()) == 0
    ref, ref_lse = sr.masked_attention_fp64(q, k, v, heads, mask, scale=fc.SCALE)
    assert rel_l2(got.cpu(), ref) < 5e-3 and float((lse.cpu().double() - ref_lse).abs().max()) < 2e-2
    # overflow inside a listed tile: the first listed tile of query block 1 is tile 8, the rise is taken against IT
    q3, k3, v3 = fc.random_case(11, sq, skv, heads)
    real = fc.add_rise(q3, k3, fc.RISE_HEAD, fc.RISE_ROW, 1000, fc.OVERFLOW_RISE, first_keys=range(512, 576))
    assert real >= 130
    got3 = ops.flash_attn_sparse(q3.cuda(), k3.cuda(), v3.cuda(), heads, bm, scale=fc.SCALE)
    flags = ops.last_attn_flags.cpu()
    want = torch.zeros_like(flags)
    want[fc.RISE_HEAD, 1, (fc.RISE_ROW % 256) // 32] = 1
    assert torch.equal(flags, want), flags.tolist()
    with ops.options(attn_fixed_max=0):
        exact3 = ops.flash_attn_sparse(q3.cuda(), k3.cuda(), v3.cuda(), heads, bm, scale=fc.SCALE)
    cols = slice(128 * fc.RISE_HEAD, 128 * fc.RISE_HEAD + 128)
    assert torch.equal(got3[256:, cols], exact3[256:, cols]) and bool(torch.isfinite(got3.float()).all())
    assert rel_l2(got3.cpu(), sr.masked_attention_fp64(q3, k3, v3, heads, mask, scale=fc.SCALE)[0]) < 5e-3


def test_option_off_is_the_exact_entry_point_bit_for_bit(ops):
    from goal_force_amd import _lib
    sq, skv, heads = 300, 2100, 3
    q, k, v = (t.cuda() for t in fc.random_case(3, sq, skv, heads))
    with ops.options(attn_fixed_max=0):
        off = ops.flash_attn(q, k, v, heads, scale=fc.SCALE)
        assert ops.last_attn_flags is None
    lib, st, kvp = _lib.load(), torch.cuda.current_stream().cuda_stream, ops.kv_pad(skv)
    vt = torch.empty((heads * 128 * kvp,), dtype=BF, device="cuda")
    want = torch.empty_like(q)
    _lib.check(lib.gf_transpose_v32(v.data_ptr(), v.stride(0), vt.data_ptr(), skv, kvp, heads, st), "gf_transpose_v32")
    _lib.check(lib.gf_flash_attn_fwd_vt32(q.data_ptr(), k.data_ptr(), vt.data_ptr(), want.data_ptr(), None, sq, skv, kvp, heads, 128,
                                          q.stride(0), k.stride(0), want.stride(0), fc.SCALE, st), "gf_flash_attn_fwd_vt32")
    assert torch.equal(off, want)
    # the _fm entry point under the option: the same single exact launch, flags zeroed
    flags = torch.full((heads * 2 * 8,), 7, dtype=torch.int32, device="cuda")
    got = torch.empty_like(q)
    with ops.options(attn_fixed_max=0):
        _lib.check(lib.gf_flash_attn_fwd_vt32_fm(q.data_ptr(), k.data_ptr(), vt.data_ptr(), got.data_ptr(), None, flags.data_ptr(), sq, skv, kvp,
                                                 heads, 128, q.stride(0), k.stride(0), got.stride(0), fc.SCALE, st), "gf_flash_attn_fwd_vt32_fm")
    assert torch.equal(got, want) and int(flags.count_nonzero()) == 0
    assert ops.lib_option("attn_fixed_max") == 1
