"""The CPU proof of tests/sage_refs.py (no GPU): the fp32 restatement of the SageAttention kernel's path passes the exact classes with
equality and both bars on every gauss input of tests/test_sage_pinned_gpu.py; each injected fault breaks an exact class or is outside
a named bar; which of them the old whole-tensor rel-L2 of 5e-4 passes is printed and asserted (`pytest -s`)."""
import math

import pytest
import torch

import gemm_refs as G
import sage_oracle as so
import sage_refs as R

BF = torch.bfloat16
OLD_BAR = 5e-4                                             # tests/test_sage_attention_gpu.py


def _f64_exact(op):
    """bf16 of the fp64 recipe on exact sums, and the model's bits: equal on an exact class."""
    ref = R.recipe(op)
    return ref.out.to(BF), ref.model, ref


def test_pow2_scales_and_positions():
    for k in range(8):
        R.pow2_scale(k)
    pos = so.vt_position(513)
    assert sorted(pos.tolist()) == list(range(513)) and int(pos[128]) == 128 and int(pos[4]) == 32 and int(pos[16]) == 4
    assert len(R.FINITE) == 254 and bool(torch.isfinite(R.decode(R.FINITE)).all())


@pytest.mark.parametrize("where", ["first", "last", "spread"])
def test_one_hot_restated_exactly(where):
    for q_len, kv, heads, shift in R.ONE_HOT_CASES + ((129, 513, 3, 0), (33, 97, 3, 64)):
        op, hot, want = R.one_hot(q_len, kv, heads, where, shift)
        got = R.restate(op)
        msg = R.one_hot_report(got, op, hot, want, shift)
        assert msg is None, msg
        if (q_len, kv) == (129, 513):
            exact, model, _ = _f64_exact(op)
            assert torch.equal(exact.float(), want.float()) and torch.equal(model.float(), want.float())
            if where == "first":
                assert len(set((so.vt_position(kv)[hot[0]] % 128).tolist())) == 128, "head 0's hot keys miss a position of the slice"
    op, hot, want = R.one_hot(129, 513, 3, "spread")
    assert {63, 64, 127, 128} <= set(hot[0].tolist()) and int(hot[2, 0]) == 512 and int(hot[1, 0]) // 128 == 2


def test_uniform_restated_exactly():
    for kv in R.UNIFORM_KV:
        for variant in ("q0", "qs0", "ks0"):
            op, want = R.uniform(33, kv, 2, variant, garbage=(kv % 3 == 0))
            assert torch.equal(R.restate(op).float(), want.float()), (kv, variant)
    op, want = R.uniform(33, 97, 2, "ks0", garbage=True)
    exact, model, _ = _f64_exact(op)
    assert torch.equal(exact.float(), want.float()) and torch.equal(model.float(), want.float())


def test_staircase_is_exact_in_fp32():
    """Nothing rounds before the tail: the restatement equals bf16 of the fp64 recipe on exact sums, and mfma_fp8 truncates nothing."""
    for nt in (2, 3, 4, 5):
        for kv in (128 * nt, 128 * nt - 61):
            op = R.staircase(129, nt, 3, kv)
            exact, model, ref = _f64_exact(op)
            got = R.restate(op)
            assert torch.equal(got.float(), R.exact_tail(op, ref).float()) and torch.equal(model.float(), exact.float()), (nt, kv)
            assert not bool(ref.excused.any())


def _gauss_op(sq, skv, heads, std, blocks=True):
    return R.quantise(*R.gauss_qkv(sq, skv, heads, std, 0, blocks), heads)


def test_restatement_inside_both_bars_on_every_gauss_input():
    worst = dict(share=0.0, worst=0.0, excused=0.0)
    for sq, skv, heads, std, blocks in R.gauss_cases():
        op = _gauss_op(sq, skv, heads, std, blocks)
        j = R.assert_pinned(R.restate(op), R.recipe(op), f"restatement gauss q={sq} keys={skv} heads={heads} std={std} blocks={blocks}")
        worst = {k: max(worst[k], j[k]) for k in worst}
    print(f"RESTATEMENT gauss: worst differing share {worst['share']:.2e} (cap {G.SHARE_CAP:.2e}), worst ratio of (b) {worst['worst']:.3f}, "
          f"largest excused share {100 * worst['excused']:.2f} % (cap 2 %)")
    assert worst["share"] <= G.SHARE_CAP / 2, "the restatement's own share is above half the cap: the GPU test must use twice it"


def _fault_case(fault):
    """(op the fault runs on, the exact class's expectation (None: exact_tail of the recipe's sums), exact?)"""
    if fault in ("intmin_only",):
        op, _ = R.uniform(33, 97, 2, "ks0", garbage=True)
        return op, None, True
    if fault in ("drop_last_key", "one_past"):
        op, _ = R.uniform(33, 97, 2, "q0")
        return op, None, True
    if fault in ("k_scale_next", "q_scale_next", "alpha_one_qb", "rescale_skips_l"):
        op = R.staircase(129, 3, 3)
        return op, None, True
    if fault == "vt_natural":
        op, _, want = R.one_hot(129, 257, 3, "spread")
        return op, want, True
    if fault == "no_hvalid":
        op, _ = R.uniform(33, 130, 2, "q0", garbage=True)
        return op, None, True
    op = _gauss_op(129, 97, 3, 1.0, False)
    if fault == "keep_only":
        g = torch.Generator().manual_seed(3)
        op.k8[97:] = torch.randint(-127, 128, (31, 3 * 128), generator=g).to(torch.int8)
    return op, None, False


@pytest.mark.parametrize("fault", R.FAULTS)
def test_injected_fault_is_caught(fault):
    op, want, exact = _fault_case(fault)
    right, wrong = R.restate(op), R.restate(op, fault)
    ref = R.recipe(op)
    old = R.rel_l2(wrong, ref.out.to(BF))
    if exact:
        assert torch.equal(right.float(), (R.exact_tail(op, ref) if want is None else want).float())
        caught = not torch.equal(wrong.float(), right.float())
        how = "breaks the exact class"
    else:
        assert not R.failed_bars(R.judge(right, ref))
        bad = R.failed_bars(R.judge(wrong, ref))
        caught, how = bool(bad), f"outside {bad}"
    print(f"FAULT {fault}: {how}; old rel-L2 {old:.2e} ({'passes' if old <= OLD_BAR else 'fails'} the old 5e-4)")
    assert caught, fault


def test_input_faults_are_caught():
    """One V key row 5 % off at 97 keys; the neighbouring 64-key half's k_scale and the next Q block's q_scale on gauss operands (whose
    blocks differ by 2^6); the vt32 halves exchanged in the V^T producer."""
    q, k, v = R.gauss_qkv(129, 97, 3, 1.0)
    op = R.quantise(q, k, v, 3)
    ref = R.recipe(op)
    v2 = v.clone()
    v2[96] = (v2[96].float() * 1.05).to(BF)
    wrong = R.restate(R.quantise(q, k, v2, 3))
    bad = R.failed_bars(R.judge(wrong, ref))
    old = R.rel_l2(wrong, ref.out.to(BF))
    print(f"FAULT v_row_5pct at 97 keys: outside {bad}; old rel-L2 {old:.2e} ({'passes' if old <= OLD_BAR else 'fails'} the old 5e-4)")
    assert bad
    for fault in ("k_scale_next", "q_scale_next", "row_2pct", "l_unquantised", "v_scale_next_head"):
        wrong = R.restate(op, fault)
        bad = R.failed_bars(R.judge(wrong, ref))
        old = R.rel_l2(wrong, ref.out.to(BF))
        print(f"FAULT {fault} on gauss: outside {bad}; old rel-L2 {old:.2e} ({'passes' if old <= OLD_BAR else 'fails'} the old 5e-4)")
        assert bad, fault
    op = _gauss_op(2049, 129, 1, 1.0, False)
    ref, wrong = R.recipe(op), R.restate(op, "row_2pct")
    bad, old = R.failed_bars(R.judge(wrong, ref)), R.rel_l2(wrong, ref.out.to(BF))
    print(f"FAULT row_2pct, one row in 2049: outside {bad}; old rel-L2 {old:.2e} ({'passes' if old <= OLD_BAR else 'fails'} the old 5e-4)")
    assert bad and old <= OLD_BAR, "one row in 2049 that is 2 % off passes the old bar and not the new ones"
    for kv in (33, 97, 257):
        vv = R.gauss_qkv(1, kv, 2, 1.0)[2]
        vt32 = R.vt32_of(vv)
        vt32[:, G.vt_positions(vt32.shape[1])[kv:]] = math.nan
        want8, wants = R.quant_vt_ref(vv, 2)
        got8, gots = R.vt32_producer(vt32, kv, 2)
        assert torch.equal(got8, want8) and torch.equal(gots, wants)
        bad8, _ = R.vt32_producer(vt32, kv, 2, "halves_exchanged")
        assert not torch.equal(bad8, want8), kv


def test_tiny_blocks_in_the_oracle():
    """The header's tiny-block rule as sage_oracle restates it: finite codes, code 0 for a zero element, no e4m3 NaN code, a product
    code x scale within the code's rounding of the element; blocks from 2^-100 up unchanged."""
    for amax in R.TINY:
        x = R.tiny_rows(64, 2, amax)
        c, s = so.quant_int8(x.float().view(64, 2, 128).transpose(0, 1), 32)
        assert bool((c[x.view(64, 2, 128).transpose(0, 1) == 0] == 0).all()) and bool(torch.isfinite(s).all()) and bool((s > 0).all())
        v8, vs = so.quant_v(x, 2)
        codes = v8.view(torch.uint8)
        assert not bool(((codes & 0x7F) == 0x7F).any()) and bool((codes[x.view(64, 2, 128).transpose(0, 1) == 0] & 0x7F == 0).all())
        back = v8.float().double() * vs.double()[:, None, :]
        assert bool(((back - x.double().view(64, 2, 128).transpose(0, 1)).abs() <= 2.0 ** -4 * amax + 2.0 ** -140).all()), amax
    x = (torch.randn((64, 256), generator=torch.Generator().manual_seed(1)) * 2.0 ** -100).to(BF)
    amax = x.float().view(64, 2, 128).transpose(0, 1).abs().amax(1)
    assert torch.equal(so.quant_v(x, 2)[1], amax / torch.tensor(448.0))
