"""CPU evidence for tests/attention_bwd_refs.py, the yardstick of tests/test_attention_bwd_gpu.py: the fp64 reference agrees with torch's
own attention, a RIGHT fp32 restatement of the kernels' chain is inside the element bound and the row bar on every shape and data class
the GPU tests run, and each injected fault is outside — while the whole-tensor rel-L2 bar used before (1e-2) lets a key row of dK that is
5 % off through."""
import math

import pytest
import torch

import attention_bwd_refs as R

FAULT_CASES = [("std1", 257, 193, 3), ("std1", 97, 145, 3)]       # ragged in every kernel's tile; three heads (lse_transposed needs > 1)


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _case(case):
    name, sq, skv, heads = case
    q, k, v, dout, scale = R.case_inputs(name, sq, skv, heads, torch.Generator().manual_seed(R.case_seed(*case)))
    ref = R.grads_ref(q, k, v, dout, heads, scale)
    return (q, k, v, dout, scale), ref


def _chain(inp, ref, fault=None):
    q, k, v, dout, scale = inp
    o, lse = R.kernel_inputs(ref)
    return R.chain_f32(q, k, v, o, dout, lse, ref.heads, scale, fault=fault)


@pytest.fixture(scope="module")
def fault_cases():
    return [_case(c) for c in FAULT_CASES]


@pytest.mark.parametrize("sq,skv,heads", [(40, 70, 2), (129, 65, 3)])
def test_grads_ref_equals_fp32_autograd_of_sdpa(sq, skv, heads):
    g = torch.Generator().manual_seed(sq)
    q, k, v, dout, scale = R.case_inputs("std1", sq, skv, heads, g)
    ref = R.grads_ref(q, k, v, dout, heads, scale)
    with torch.enable_grad():
        qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
        h = lambda t: t.view(t.shape[0], heads, R.HD).transpose(0, 1)[None]        # noqa: E731
        o = torch.nn.functional.scaled_dot_product_attention(h(qf), h(kf), h(vf))[0].transpose(0, 1).reshape(sq, heads * R.HD)
        o.backward(dout.float())
    for name, a, b in (("o", o.detach(), ref.o), ("dq", qf.grad, ref.dq), ("dk", kf.grad, ref.dk), ("dv", vf.grad, ref.dv)):
        assert R.rel_l2(a, b) < 2e-6, (name, R.rel_l2(a, b))
    s = scale * torch.einsum("qhd,khd->qhk", q.double().view(sq, heads, R.HD), k.double().view(skv, heads, R.HD))
    assert float((ref.lse2 - torch.logsumexp(s, -1) * R.LOG2E).abs().max()) < 1e-12
    # the intermediates the bounds are built from restate the gradients they belong to
    K, Q = (t.double().view(-1, heads, R.HD).transpose(0, 1) for t in (k, q))
    assert R.rel_l2(R._flat(scale * ref.dS @ K), ref.dq) < 1e-12 and R.rel_l2(R._flat(scale * ref.dS.transpose(1, 2) @ Q), ref.dk) < 1e-12
    assert float(ref.P.sum(-1).sub(1).abs().max()) < 1e-12


def test_covering_pairs_meet_every_length_twice():
    assert 50 <= len(R.TILE_PAIRS) <= 60 and len(set(R.TILE_PAIRS)) == len(R.TILE_PAIRS)
    for qv in R.Q_LENS:
        assert len({kv for sq, kv in R.TILE_PAIRS if sq == qv}) >= 2, qv
    for kv in R.KV_LENS:
        assert len({sq for sq, skv in R.TILE_PAIRS if skv == kv}) >= 2, kv


def test_right_chain_is_inside_both_bars_on_every_gpu_case():
    """Every case of the GPU tests: no element outside, and the worst row ratio IS what the helper states (ROW_CHAIN_WORST, from which
    the kernels' bar is 1.25 x) — measured here, so the figure in the helper cannot go stale."""
    worst_e, worst_r = 0.0, {"far": 0.0, "rest": 0.0}
    for case in R.all_cases():
        inp, ref = _case(case)
        got = _chain(inp, ref)
        for name, t in zip(("dq", "dk", "dv"), got):
            n, we, wr = R.measure(t, ref, name)
            assert n == 0, (case, name, n, we)
            grp = "far" if case[0].startswith("far_") else "rest"
            worst_e, worst_r[grp] = max(worst_e, we), max(worst_r[grp], wr)
    print(f"right chain over {len(R.all_cases())} cases: worst element {worst_e:.3f} of the allowance, worst row ratio {worst_r}")
    assert worst_e <= 1.0
    for grp, w in worst_r.items():
        assert 0.95 * R.ROW_CHAIN_WORST[grp] <= w <= R.ROW_CHAIN_WORST[grp], (grp, w, R.ROW_CHAIN_WORST[grp])


def test_the_conditions_the_gpu_cases_rely_on():
    """far_below: lse < -130 (the padded keys' exp2(-lse) overflows); far_above: lse > +130; kv_len = 1: dq = dk = 0; v_const: dS = 0;
    delta0: delta exactly 0 on every third query and not elsewhere."""
    for sq, skv in R.CLASS_SHAPES + [R.FAR_BELOW_CONTROL]:
        assert float(_case(("far_below", sq, skv, 2))[1].lse2.max()) < -130
    for sq, skv in R.CLASS_SHAPES:
        assert float(_case(("far_above", sq, skv, 2))[1].lse2.min()) > 130
        ref = _case(("v_const", sq, skv, 2))[1]
        assert float(ref.dS.abs().max()) < 1e-12 and float(ref.dq.abs().max()) < 1e-12 and float(ref.dv.abs().max()) > 0.1
        ref = _case(("delta0", sq, skv, 2))[1]
        assert float(ref.delta[:, ::3].abs().max()) == 0.0 and float(ref.delta[:, 1::3].abs().min()) > 0
    assert R.FAR_BELOW_CONTROL[1] % 64 == 0 and all(skv % 64 for _, skv in R.CLASS_SHAPES)
    ref = _case(("std1", 97, 1, 3))[1]
    assert float(ref.dq.abs().max()) < 1e-12 and float(ref.dk.abs().max()) < 1e-12


@pytest.mark.parametrize("fault", ["dk_row_5pct", "dq_drops_last_key", "delta_from_row_plus_32", "lse_transposed"])
def test_fault_fails_the_element_bound(fault_cases, fault):
    hit = {"dk_row_5pct": ("dk",), "dq_drops_last_key": ("dq",), "delta_from_row_plus_32": ("dq", "dk"), "lse_transposed": ("dq", "dk", "dv")}
    for inp, ref in fault_cases:
        got = _chain(inp, ref, fault)
        for name, t in zip(("dq", "dk", "dv"), got):
            n, we, _ = R.measure(t, ref, name)
            print(f"{fault} {name}: {n} elements outside, worst {we:.2f}x the allowance")
            assert (n > 0 and we > 1.5) if name in hit[fault] else n == 0, (fault, name, n, we)
        with pytest.raises(AssertionError, match="outside the bound"):
            R.assert_within(got, ref, fault)


def test_whole_tensor_bar_is_blind_to_a_key_row_5_percent_off(fault_cases):
    """Why the old bars were not enough: the faulty dK passes rel-L2 < 1e-2 (and the 5e-3 of the ragged test) on the whole tensor."""
    for inp, ref in fault_cases:
        dk = _chain(inp, ref, "dk_row_5pct")[1]
        e = R.rel_l2(dk, ref.dk)
        print(f"dk with one key row 5 % off: rel-L2 {e:.2e}; the right chain {R.rel_l2(_chain(inp, ref)[1], ref.dk):.2e}")
        assert e < 5e-3 < 1e-2
        assert R.measure(dk, ref, "dk")[0] > 0


def test_second_rounding_and_a_2_percent_row_fail_the_row_bar(fault_cases):
    """What the element bound cannot see: dS built from the rounded P passes it and fails the row bar on dq (dk comes to 2.2, just
    under: a second rounding adds at most a factor sqrt(2) to noise whose worst row already is 1.4 - 1.9); one row of one head 2 % off
    fails it on each gradient by a factor of three or more."""
    inp, ref = fault_cases[0]
    bar = R.row_bar("std1")
    got = _chain(inp, ref, "ds_from_rounded_p")
    for name, t in zip(("dq", "dk", "dv"), got):
        n, we, wr = R.measure(t, ref, name)
        print(f"ds_from_rounded_p {name}: {n} elements outside, worst row {wr:.2f} (bar {bar:.2f})")
        assert n == 0 and (wr > bar if name == "dq" else wr > 0), (name, n, wr)
    with pytest.raises(AssertionError, match="predicted rounding noise"):
        R.assert_within(got, ref, "ds_from_rounded_p")
    for inp, ref in fault_cases:
        for name, t in zip(("dq", "dk", "dv"), _chain(inp, ref)):
            t = t.clone()
            row = t.shape[0] // 2
            t[row, :R.HD] = (t[row, :R.HD].float() * 1.02).to(R.BF)
            wr = R.measure(t, ref, name)[2]
            print(f"one row of {name} 2 % off: worst row {wr:.2f} (bar {bar:.2f})")
            assert wr > 2 * bar, (name, wr)


def test_non_finite_results_count_as_outside(fault_cases):
    inp, ref = fault_cases[1]
    for bad in (math.nan, math.inf):
        got = [t.clone() for t in _chain(inp, ref)]
        got[0][3, 5] = bad
        assert R.measure(got[0], ref, "dq") == (1, math.inf, math.inf)
        with pytest.raises(AssertionError):
            R.assert_within(got, ref, "non-finite")


def test_embed_is_a_view_into_a_filled_buffer():
    t = torch.arange(12, dtype=torch.float32).view(3, 4).to(R.BF)
    e = R.embed(t, 2, 8)
    assert torch.equal(e, t) and e.stride(0) == 12 and not e.is_contiguous()
    assert e.untyped_storage().nbytes() == 5 * 12 * 2
    whole = torch.as_strided(e, (5, 12), (12, 1))
    assert int(torch.isnan(whole.float()).sum()) == 5 * 12 - 12
