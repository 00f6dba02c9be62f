"""CPU evidence for tests/attention_fwd_refs.py, the yardstick of tests/test_attention_fwd_gpu.py: the fp64 reference agrees with torch's
own attention, the RIGHT fp32 restatement of each forward kernel is inside the element bound, the lse bound and the row bar on every
case the GPU test runs, the measured worst row ratios ARE the helper's constants, and each injected fault is outside at least one bar
at the smallest shape where it applies.

What each fault measures (the case in FAULT_CASES; element = worst error over the allowance, row = worst row ratio over the bar in
force, lse in log2 units), and whether the bars used before — rel-L2 < 4e-3 on the whole tensor, |lse - ref| < 2e-2 — let it through:
    fault                   kernel 2                                     kernel 3 (exact; fixed maximum alike)          old bars
    v_row_5pct              element 6.4 x, row 20.9                       element 1.6 x, row 16.6                        rel-L2 5.1e-3 at 33 keys: caught; 2.3e-3 at 97 keys: PASSED
    drops_last_key          element 460 x, lse off by 2.0                 element 16 x, lse off by 0.62                  caught (0.07 - 0.13)
    reads_one_past          element 104 x, lse off by 0.80                element 1.6 x on 780 elements, row 69, lse     kernel 2 caught (4.4e-2); kernel 3 caught on far_below only:
                                                                          off by 194 (far_below: the zero key scores 0,   on std3 data the zero key changes 3.2e-3 -> 3.2e-3, PASSED
                                                                          200 above every real one)
    vt_group_unswapped      element 2.6e4 x                               element 2.1e3 x                                caught (0.96)
    l_from_unrounded_p      (kernel 2's own arithmetic: no fault)         fixed maximum, v_const: 209 elements a whole   PASSED (2.0e-3 against 1.8e-3 for the right chain)
                                                                          ulp off (1.3 x); exact, prescaled: 9 elements
                                                                          1.24 x, row 2.08 against the bar 2.15: the elements alone — the
                                                                          running maximum's top key has p = 1 exactly,
                                                                          which hides the fault where one key dominates
    rescale_skips_l         element 79 x, lse off by 1.4 (rise_mid)       element 158 x, lse off by 1.4 (rise_mid)       caught on a rise (0.19); no random case has one
    lse_natural_log         lse off by 4.9                                lse off by 6.5                                 caught (the old lse tests ran at two shapes)
    lse_transposed          lse off by 7.9                                lse off by 10                                  caught
    lastmult_on_wrong_key   element 86 x at multiplicity 2                (kernel 2 only)                                caught (0.18)
    row_2pct                element 2.7 x, row 8.8                        element inside (0.77), row 4.9 against 2.93    PASSED (2.1e-3 / 3.4e-3 against 1.7e-3 / 3.2e-3)
"""
import math

import numpy as np
import pytest
import torch

import attention_fwd_refs as R
import attn_fixed_max_cases as fc

K2_SMALL, K3_SMALL = ("std3", 65, 33, 3, 1), ("std3", 65, 129, 3, 1)
RISE_CASE = ("rise_mid", *R.CLASS_SHAPE, R.CLASS_HEADS, 1)
# fault -> kind -> (class, q_len, kv_len, heads, multiplicity): the smallest shape at which the fault applies
FAULT_CASES = {
    "v_row_5pct": {"k2": K2_SMALL, "k3": K3_SMALL, "k3fm": K3_SMALL},
    "drops_last_key": {"k2": K2_SMALL, "k3": K3_SMALL, "k3fm": K3_SMALL},
    "reads_one_past": {"k2": K2_SMALL, "k3": ("far_below", 65, 129, 3, 1), "k3fm": ("far_below", 65, 129, 3, 1)},
    "vt_group_unswapped": {"k2": K2_SMALL, "k3": K3_SMALL, "k3fm": K3_SMALL},
    "l_from_unrounded_p": {"k3": ("prescaled", 65, 161, 3, 1), "k3fm": ("v_const", 65, 129, 3, 1)},
    "rescale_skips_l": {"k2": RISE_CASE, "k3": RISE_CASE},            # needs a maximum that moves after tile 0
    "lse_natural_log": {"k2": K2_SMALL, "k3": K3_SMALL, "k3fm": K3_SMALL},
    "lse_transposed": {"k2": K2_SMALL, "k3": K3_SMALL, "k3fm": K3_SMALL},
    "lastmult_on_wrong_key": {"k2": ("std1", 65, 33, 2, 2)},
    "row_2pct": {"k2": K2_SMALL, "k3": K3_SMALL, "k3fm": K3_SMALL},
}
OLD_REL_L2, OLD_LSE = 4e-3, 2e-2
# (fault, kind) the old whole-tensor bars let through on FAULT_CASES — the docstring's last column
OLD_BARS_PASS = {("l_from_unrounded_p", "k3"), ("l_from_unrounded_p", "k3fm"), ("row_2pct", "k2"), ("row_2pct", "k3"), ("row_2pct", "k3fm")}


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


_CACHE = {}


def _case(name, sq, skv, heads, mult=1, mp=None):
    key = (name, sq, skv, heads, mult, mp)
    if key not in _CACHE:
        q, k, v, scale = R.case_inputs(name, sq, skv, heads)
        sel = None
        if mp is not None:
            sel = R.selection(*R.sparse_map(mp, sq, skv, heads), heads, sq, skv)
        _CACHE[key] = ((q, k, v, scale, sel), R.attn_ref(q, k, v, heads, scale, mult, sel))
    return _CACHE[key]


def _chain(inp, ref, kind, fault=None):
    q, k, v, scale, sel = inp
    return R.chain_f32(q, k, v, ref.heads, scale, kind, ref.mult, sel, fault=fault)


@pytest.mark.parametrize("sq,skv,heads", [(40, 70, 2), (129, 65, 3)])
def test_attn_ref_equals_sdpa_and_its_own_parts(sq, skv, heads):
    inp, ref = _case("std1", sq, skv, heads)
    q, k, v, scale, _ = inp
    h = lambda t: t.float().view(t.shape[0], heads, R.HD).transpose(0, 1)[None]        # noqa: E731
    o = torch.nn.functional.scaled_dot_product_attention(h(q), h(k), h(v))[0].transpose(0, 1).reshape(sq, heads * R.HD)
    assert R.rel_l2(o, ref.o) < 2e-6
    s = scale * torch.einsum("qhd,khd->qhk", q.double().view(sq, heads, R.HD), k.double().view(skv, heads, R.HD))
    assert float((ref.lse2 - torch.logsumexp(s, -1) * R.LOG2E).abs().max()) < 1e-12
    assert float(ref.P.sum(-1).sub(1).abs().max()) < 1e-12
    assert R.rel_l2(R._flat(ref.P @ R._heads(v.double(), heads)), ref.o) < 1e-14
    D = R.spread(ref, ref.P)
    i, d = sq // 2, 77
    want = (ref.P[1, i] * (v.double()[:, R.HD + d] - ref.o[i, R.HD + d]).abs()).sum()
    assert abs(float(D[1, i, d] - want)) < 1e-12 and float(D.min()) >= 0


def test_multiplicity_is_the_keys_written_out_and_selection_is_the_softmax_over_the_selected_keys():
    q, k, v, scale = R.case_inputs("std1", 33, 65, 2)
    m = 5
    ref = R.attn_ref(q, k, v, 2, scale, mult=m)
    kk, vv = (torch.cat([t, t[-1:].expand(m - 1, -1)]) for t in (k, v))
    long = R.attn_ref(q, kk, vv, 2, scale)
    assert torch.equal(ref.o, long.o) and torch.equal(ref.lse2, long.lse2)
    assert float((ref.P[:, :, -1] - long.P[:, :, 64:].sum(-1)).abs().max()) < 1e-15 and float(ref.P.sum(-1).sub(1).abs().max()) < 1e-12
    sq, skv, heads = R.SPARSE_SHAPE
    for name in R.SPARSE_MAPS:
        lists, hm = R.sparse_map(name, sq, skv, heads)
        nt = -(-skv // 64)
        assert all(row == sorted(set(row)) and row and 0 <= row[0] and row[-1] < nt for mp in lists for row in mp), name
        rp, ti = R.csr(lists)
        assert rp.dtype == ti.dtype == torch.int32 and int(rp[-1]) == ti.numel() and rp.numel() == len(lists) * 2 + 1
        (q, k, v, scale, sel), ref = _case("std1", sq, skv, heads, 1, name)
        keys = sel[2][1]                                                               # head 2, query block 1
        part = R.attn_ref(q[256:, 256:], k[keys][:, 256:], v[keys][:, 256:], 1, scale)
        assert R.rel_l2(part.o, ref.o[256:, 256:]) < 1e-14 and float(ref.P[2, 256:].sum(-1).sub(1).abs().max()) < 1e-12
    assert R.sparse_map("one_tile", sq, skv, heads)[0][0][0] == [nt - 1] and R.sparse_map("ends_ragged", sq, skv, heads)[0][0][1][-1] == nt - 1
    assert all(row[-1] < nt - 1 for row in R.sparse_map("skips_ragged", sq, skv, heads)[0][0])
    assert len(R.sparse_map("two_maps", sq, skv, heads)[0]) == 2 and R.sparse_map("two_maps", sq, skv, heads)[1] == [1, 0, 1]


def test_the_case_lists_cover_what_they_claim():
    for pairs, kvs in ((R.K2_PAIRS, R.K2_KV), (R.K3_PAIRS, R.K3_KV)):
        assert {kv for _, kv in pairs} == set(kvs) and {sq for sq, _ in pairs} == set(R.Q_LENS) and len(pairs) == len(kvs)
    assert {kv % 64 for kv in R.K3_KV} >= {0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63}
    assert {-(-kv // 64) for kv in R.K3_KV} == set(range(2, 10)) and min(R.K3_KV) == 128
    assert all(h % 8 == 0 and sq > 256 for sq, _, h in R.K2_XCD + R.K3_XCD)
    assert R.CLASS_SHAPE[1] % 64 and R.CLASS_SHAPE[0] > 256 and R.FAR_BELOW_CONTROL[1] % 64 == 0
    assert (97 - 1) % 64 >= 32 and 97 in R.MULT_KV


def test_scale_ln2_makes_kernel_3s_factor_exactly_one():
    """fp32(ln 2) x fp32(log2 e) rounds to 1.0f: the pre-scaled q is not rounded a second time, and its bound has no s_ij."""
    assert np.float32(fc.SCALE) * np.float32(R.LOG2E) == np.float32(1.0) and R.factor(fc.SCALE) == 1.0
    assert R.bound_class("k3", fc.SCALE) == "k3" and R.bound_class("k3fm", 1 / math.sqrt(128)) == "k3q" and R.factor(1 / math.sqrt(128)) != 1.0
    q = R.case_inputs("prescaled", 33, 129, 1)[0]
    assert torch.equal((q.float() * R.factor(fc.SCALE)).to(R.BF), q)
    assert abs(fc.C * math.sqrt(128) / R.LOG2E - 1) < 1e-7


def test_right_chains_are_inside_every_bound_on_every_gpu_case():
    """Every case of the GPU test, each kernel's own restatement: no element and no lse outside, and the worst row ratio per bound
    class IS what the helper states (ROW_CHAIN_WORST; the kernels' bar is 1.25 x) — measured here, so it cannot go stale."""
    worst_e, worst_l, worst_r = 0.0, 0.0, {c: 0.0 for c in R.ROW_CHAIN_WORST}
    for kind, name, sq, skv, heads, mult, mp in R.all_cases():
        inp, ref = _case(name, sq, skv, heads, mult, mp)
        o, lse = _chain(inp, ref, kind)
        n, we, wr = R.measure(o, ref, kind)
        nl, wl, _ = R.measure_lse(lse, ref, kind)
        assert n == 0 and nl == 0, (kind, name, sq, skv, heads, mult, mp, n, we, nl, wl)
        cls = R.bound_class(kind, inp[3])
        worst_e, worst_l, worst_r[cls] = max(worst_e, we), max(worst_l, wl), max(worst_r[cls], wr)
    print(f"right chains over {len(R.all_cases())} cases: worst element {worst_e:.3f}, worst lse {worst_l:.3f} of the allowance, row ratios {worst_r}")
    assert worst_e <= 1.0 and worst_l <= 1.0
    for cls, w in worst_r.items():
        assert 0.98 * R.ROW_CHAIN_WORST[cls] <= w <= R.ROW_CHAIN_WORST[cls], (cls, w, R.ROW_CHAIN_WORST[cls])


def test_kernel_2s_lse_bound_has_no_rounded_row_sum_term():
    """Kernel 2 sums the fp32 p: its lse allowance is slop + fp32 terms alone — below 1e-4 log2 units at unit logit std, where kernel
    3's is 5.7e-3 and more — the right chain is inside on every kernel-2 case (the test above), and an lse 1e-3 off is far outside."""
    inp, ref = _case("std1", 65, 97, 3)
    a2, a3 = R.bounds(ref, "k2")[2], R.bounds(ref, "k3")[2]
    assert float(a2.max()) < 1e-4 and float(a3.min()) > R.LOG2E * R.U and float((a3 - a2).min()) >= R.LOG2E * R.U
    o, lse = _chain(inp, ref, "k2")
    assert R.measure_lse(lse, ref, "k2")[0] == 0 and R.measure_lse(lse + 1e-3, ref, "k2")[0] == lse.numel()
    assert R.measure_lse(lse + 1e-3, ref, "k3")[0] == 0            # (what the one bound for both kernels let through)
    for name in ("std8", "far_below"):
        assert float(R.bounds(_case(name, *R.CLASS_SHAPE, 2)[1], "k2")[2].max()) < 4e-4, name


def test_the_conditions_the_gpu_cases_rely_on():
    for shape in (R.CLASS_SHAPE, R.FAR_BELOW_CONTROL):
        assert float(_case("far_below", *shape, 2)[1].lse2.max()) < -180
    assert float(_case("far_above", *R.CLASS_SHAPE, 2)[1].lse2.min()) > 180
    (q, k, v, scale, _), ref = _case("v_const", *R.CLASS_SHAPE, 2)
    assert torch.equal(ref.o.float().to(R.BF), v[:1].expand_as(q)) and float(R.spread(ref, ref.P).abs().max()) < 1e-12
    assert float(_case("k_zero", *R.CLASS_SHAPE, 2)[1].P.sub(1 / R.CLASS_SHAPE[1]).abs().max()) < 1e-15
    ref = _case("one_hot", *R.CLASS_SHAPE, 2)[1]
    assert float(ref.P[:, list(R.ONE_HOT_ROWS), R.ONE_HOT_KEY].min()) > 1 - 2.0 ** -50
    for name, tile in (("rise_mid", 1), ("rise_last", 2)):
        (q, k, v, scale, _), ref = _case(name, *R.CLASS_SHAPE, 2)
        s = fc.scores(q, k, R.RISE_HEAD)[R.RISE_ROW]
        assert R.RISE_KEYS[name] // 64 == tile and int(s.argmax()) == R.RISE_KEYS[name] and 59 < float(s.max() - s[:64].max()) < 61
    assert float(_case("std1", 17, 1, 3)[1].P.min()) == 1.0


def _bars(o, lse, ref, kind, scale):
    n, we, wr = R.measure(o, ref, kind)
    nl, wl, el = R.measure_lse(lse, ref, kind)
    return dict(element=n > 0, row=wr > R.row_bar(kind, scale), lse=nl > 0), (n, we, wr, nl, wl, el)


@pytest.mark.parametrize("fault", list(R.FAULTS))
def test_every_fault_is_outside_a_bar_where_the_right_chain_is_inside(fault):
    assert set(FAULT_CASES[fault]) == set(R.FAULTS[fault])
    for kind, case in FAULT_CASES[fault].items():
        inp, ref = _case(*case)
        right = _chain(inp, ref, kind)
        out, _ = _bars(*right, ref, kind, inp[3])
        assert not any(out.values()), (fault, kind, "the right chain", out)
        o, lse = _chain(inp, ref, kind, fault)
        out, fig = _bars(o, lse, ref, kind, inp[3])
        # (the old lse bar is asked only where the right chain meets it: at logit std 8 the second rounding of q alone moves lse by 0.08)
        lse_err = lambda t: float(torch.nan_to_num((t.double() - ref.lse2).abs(), nan=math.inf).max())          # noqa: E731
        old_passes = R.rel_l2(o, ref.o) < OLD_REL_L2 and (lse_err(lse) < OLD_LSE or lse_err(right[1]) >= OLD_LSE)
        print(f"{fault} {kind} {case}: {fig[0]} elements outside (worst {fig[1]:.2f}x), row {fig[2]:.2f} (bar {R.row_bar(kind, inp[3]):.2f}), "
              f"lse {fig[3]} outside ({fig[5]:.2e}); rel-L2 {R.rel_l2(o, ref.o):.2e}: the old bars {'PASS' if old_passes else 'catch'} it")
        assert any(out.values()), (fault, kind, fig)
        assert old_passes == ((fault, kind) in OLD_BARS_PASS), (fault, kind, R.rel_l2(o, ref.o))
        with pytest.raises(AssertionError, match="outside the bound|predicted rounding noise"):
            R.assert_within(o, lse, ref, kind, fault)


def test_old_whole_tensor_bar_is_blind_at_the_old_shapes():
    """A V row 5 % off at 97 keys and a zero key read past the end of kernel 3's ragged tile on std3 data both pass rel-L2 < 4e-3;
    the first fails the row bar, the second is what far_below is for."""
    inp, ref = _case("std3", 65, 97, 3)
    o, lse = _chain(inp, ref, "k2", "v_row_5pct")
    assert R.rel_l2(o, ref.o) < OLD_REL_L2 and _bars(o, lse, ref, "k2", inp[3])[0]["row"]
    inp, ref = _case(*K3_SMALL)
    o, lse = _chain(inp, ref, "k3", "reads_one_past")
    assert R.rel_l2(o, ref.o) < OLD_REL_L2 and float((lse.double() - ref.lse2).abs().max()) < OLD_LSE
    assert not any(_bars(o, lse, ref, "k3", inp[3])[0].values())           # invisible on this data, to the new bars as well


def test_non_finite_results_count_as_outside():
    inp, ref = _case(*K2_SMALL)
    for bad in (math.nan, math.inf):
        o, lse = _chain(inp, ref, "k2")
        o[3, 5], lse[2, 1] = bad, bad
        assert R.measure(o, ref, "k2") == (1, math.inf, math.inf) and R.measure_lse(lse, ref, "k2")[:2] == (1, math.inf)
        with pytest.raises(AssertionError):
            R.assert_within(o, None, ref, "k2", "non-finite")


def test_embed_and_the_documented_permutations():
    t = torch.arange(12, dtype=torch.float32).view(3, 4).to(R.BF)
    e = R.embed(t, 2, 8, 16)
    assert torch.equal(e, t) and e.stride(0) == 28 and e.storage_offset() == 8
    whole = torch.as_strided(e, (5, 28), (28, 1), 0)
    assert int(torch.isnan(whole.float()).sum()) == 5 * 28 - 12
    assert R.vt_positions(32, 16).tolist() == [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15] + [16 + x for x in (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)]
    p32 = R.vt_positions(64, 32)
    assert p32[:16].tolist() == [0, 1, 2, 3, 16, 17, 18, 19, 4, 5, 6, 7, 20, 21, 22, 23] and sorted(p32.tolist()) == list(range(64))
    assert p32[32:40].tolist() == [32, 33, 34, 35, 48, 49, 50, 51]
