"""tests/tape_refs.py on the CPU: the order-1 restatement of the training tape is inside every bar the GPU test (test_tape_gpu.py) applies,
each injected fault is outside a named one, the whole-tensor bars the suite had before pass three of the faults, and ROW_WORST — the
figure the device's bars are 1.25 x of — reproduces.  `pytest -s` prints every figure."""
import functools

import pytest
import torch

import gemm_refs as GR
import tape_refs as T

CASES = {c["name"]: c for c in T.cases()}
TINY_CASES = [n for n, c in CASES.items() if c["cfg"] == "TINY"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs, fp64 reference, forward of order 0, chain order 0, chain order 1) of a case, computed once."""
    import gen_inputs as gi
    case = CASES[name]
    inp = T.case_inputs(case, gi)
    cfg, sd, x, ctx, t_mod, dout = inp
    ref = T.with_dx(*T.block_grads_ref(cfg, sd, x, ctx, t_mod, dout, case["grid"]))
    fwd0 = T.block_fwd(cfg, sd, x, ctx, t_mod, case["grid"], 0, case["prescale"])
    c0 = T.with_dx(*T.block_bwd(fwd0, dout))
    c1 = T.with_dx(*T.block_chain(cfg, sd, x, ctx, t_mod, dout, case["grid"], 1, case["prescale"]))
    return inp, ref, fwd0, c0, c1


@functools.lru_cache(maxsize=None)
def _model(zero):
    import gen_inputs as gi
    cfg, inp = gi.TINY, gi.train_inputs()
    dit_sd, cn_sd = gi.dit_sd(cfg, seed=41), gi.controlnet_sd(cfg, 2, seed=42, zero_convs_zero=zero)
    args = (cfg, dit_sd, cn_sd, 2, inp, gi.TRAIN_TIMESTEP_ID)
    return args, T.model_grads_ref(*args), T.model_chain(*args, order=0), T.model_chain(*args, order=1)


def _applicable(fault, case, inp):
    if fault == "q_bwd_plain_table":
        return case["prescale"]                                   # without the pre-scaled table there is nothing to confuse
    if fault == "pad_row_garbage":
        return inp[2].shape[0] % 64 != 0 or inp[3].shape[0] % 64 != 0      # a pad row exists
    return True


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_block_chain_is_inside_every_bar(name):
    _, ref, _, c0, c1 = _case(name)
    T.assert_rows(c1, c0, ref, f"chain order 1, {name}")
    assert T.old_bars_pass(c1, ref) and T.old_bars_pass(c0, ref)


def test_block_chain_exact_structure_under_a_zero_gate():
    """gate_mlp (row 5) or gate_msa (row 2) exactly zero: the branch's parameter gradients and its shift / scale rows are exactly zero
    in the reference and in the restatement, the gate's own row is not."""
    import gen_inputs as gi
    case = CASES[T.BASE_CASE]
    cfg, sd, x, ctx, t_mod, dout = T.case_inputs(case, gi)
    for row, branch, rows in ((5, "ffn.", (3, 4)), (2, "self_attn.", (0, 1))):
        tz = T.zero_gate(sd, t_mod, row)
        ref = T.with_dx(*T.block_grads_ref(cfg, sd, x, ctx, tz, dout, case["grid"]))
        c0 = T.with_dx(*T.block_chain(cfg, sd, x, ctx, tz, dout, case["grid"], 0))
        c1 = T.with_dx(*T.block_chain(cfg, sd, x, ctx, tz, dout, case["grid"], 1))
        T.assert_rows(c1, c0, ref, f"chain order 1, zero gate row {row}")
        for t in (ref, c1):
            for n in T.PARAM_NAMES:
                if n.startswith(branch):
                    assert not bool(t[n].any()), (row, n)
            m = t["modulation"].reshape(6, -1)
            assert not bool(m[list(rows)].any()) and bool(m[row].any()), row


@pytest.mark.parametrize("zero", T.MODEL_CASES)
def test_model_chain_is_inside_every_bar(zero):
    _, (loss_ref, g_ref), (l0, c0), (l1, c1) = _model(zero)
    T.assert_rows(c1, c0, g_ref, f"whole tape order 1, zero_convs_zero={zero}", model=True)
    print(f"LOSS fp64 {loss_ref:.7f} order 0 {l0:.7f} order 1 {l1:.7f}")
    assert abs(l1 - loss_ref) <= T.LOSS_MARGIN * abs(l0 - loss_ref)
    if zero:
        for n, t in c1.items():
            if "zero_convs" not in n:
                assert not bool(g_ref[n].any()) and not bool(t.any()), n


def test_row_worst_reproduces():
    """ROW_WORST is the worst ratio of the order-1 restatement per tensor group over every case the GPU tests run, to within the few
    per cent the host's fp32 matmul order may move it."""
    worst = {}
    for name in CASES:
        _, ref, _, c0, c1 = _case(name)
        for k, v in T.worst_by_group(T.measure(c1, c0, ref)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    for zero in T.MODEL_CASES:
        _, (_, g_ref), (_, c0), (_, c1) = _model(zero)
        for k, v in T.worst_by_group(T.measure(c1, c0, g_ref, model=True), True).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("ROW_WORST measured:", {k: round(v, 4) for k, v in sorted(worst.items())}, "held:", T.ROW_WORST)
    assert set(worst) == set(T.ROW_WORST)
    for k, v in worst.items():
        assert abs(v / T.ROW_WORST[k] - 1.0) <= 0.05, (k, v, T.ROW_WORST[k])


# ---------------------------------------------------------------------------------------------------------------------
# the faults
@pytest.mark.parametrize("fault", [f for f in T.BLOCK_FAULTS if f != "row_eps"])
def test_each_block_fault_is_outside_a_named_bar(fault):
    seen = 0
    for name, case in CASES.items():
        inp, ref, fwd0, c0, _ = _case(name)
        if not _applicable(fault, case, inp):
            continue
        seen += 1
        bad = T.with_dx(*T.block_bwd(fwd0, inp[5], fault))
        fails = T.failures(T.measure(bad, c0, ref))
        old = T.old_bars(bad, ref)
        print(f"FAULT {fault} {name}: outside {len(fails)} bar(s), first: {fails[:1]}; the old whole-tensor bars "
              f"{'PASS it' if all(v[0] for v in old.values()) else 'fail on ' + ', '.join(n for n, v in old.items() if not v[0])}")
        assert fails, f"{fault} at {name} is inside every bar"
    assert seen


def test_row_eps_fault_is_outside_and_the_old_bars_pass_it():
    """Fault 13 on every 2-D gradient of every case: row rows/2 times 1 + eps, eps = 2 ROW_BAR x the tensor's relative row noise."""
    table = {}
    for name in CASES:
        _, ref, _, c0, c1 = _case(name)
        for n in c1:
            if n == "dx" or ref[n].dim() < 2 or n == "modulation":
                continue
            bar = T.ROW_BAR[T.group(n)]
            eps = T.row_eps(n, c0[n], ref[n], bar)
            for factor in T.EPS_FACTORS:                                   # the smallest multiple of the stated eps that is outside
                bad = dict(c1)
                bad[n] = T.apply_row_eps(c1[n], factor * eps)
                st = T.measure({n: bad[n]}, c0, ref)[n]
                if st["worst"] > bar:
                    break
            table.setdefault(n, []).append((name, eps, factor, st["worst"], bar))
            assert st["worst"] > bar, f"{n} at {name}: a row scaled by 1 + {factor} x {eps:.3e} measures {st['worst']:.3f}, bar {bar:.3f}"
            assert factor <= T.EPS_FACTOR[T.group(n)], f"{n} at {name}: eps = {eps:.3e} needs the factor {factor}"
            assert T.old_bars_pass(bad, ref), f"{n} at {name}: the old bars were expected to pass eps = {factor * eps:.3e}"
    for n, rows in table.items():
        print(f"EPS {n}: " + "  ".join(f"{c} eps {e:.3e} x {f} -> {w:.2f} (bar {b:.2f})" for c, e, f, w, b in rows))


def test_what_the_old_bars_pass():
    """The whole-tensor rel-L2 thresholds of test_training_gpu.py (2.5e-2; attn.k.bias 8e-2; dx 1.5e-2) against three faults, with the
    figures.  They pass (1) the (1 + eps) row of every weight gradient (the test above), (2) ONE ROW 50 % OFF in every 1536-row weight
    gradient of the mid case (0.5 / sqrt(1536) = 1.3e-2), and (3) the bias gradient without its last token row on self_attn.v.bias at the
    base case (1 / sqrt(72) of a gradient whose rows nearly cancel); the new bars are outside on each.  They do NOT pass the other biases
    without their last row at 72 tokens (1.2e-1 .. 4.8), nor the dropped k contribution to dh1 (modulation and dx): what the issue
    expected of them there holds only at token counts above ~1600 — recorded here as measured, not as hoped."""
    inp, ref, fwd0, c0, c1 = _case("mid-130-65")
    for n in ("self_attn.q.weight", "ffn.0.weight", "cross_attn.k.weight"):
        bad = dict(c1)
        bad[n] = T.apply_row_eps(c1[n], 0.5)
        e = T.old_bars(bad, ref)[n]
        st = T.measure({n: bad[n]}, c0, ref)[n]
        print(f"OLD row 50 % off, {n} (mid): rel-L2 {e[1]:.3e} under the old bar {e[2]:.1e}; the row statistic {st['worst']:.1f}")
        assert e[0] and st["worst"] > T.ROW_BAR[T.group(n)]
    inp, ref, fwd0, c0, _ = _case(T.BASE_CASE)
    for fault, passes in (("bias_drops_last_row", ("self_attn.v.bias",)), ("dh1_no_k", ())):
        bad = T.with_dx(*T.block_bwd(fwd0, inp[5], fault))
        old, new = T.old_bars(bad, ref), T.measure(bad, c0, ref)
        changed = [n for n in bad if not torch.equal(bad[n], c0[n])]
        for n in changed:
            bar = T.ROW_BAR[T.group(n)]
            print(f"OLD {fault} {n}: rel-L2 {old[n][1]:.3e} / old bar {old[n][2]:.1e} ({'passes' if old[n][0] else 'caught'}); "
                  f"row statistic {new[n]['worst']:.1f} / bar {bar:.2f}")
        for n in passes:
            assert old[n][0] and new[n]["worst"] > T.ROW_BAR[T.group(n)], (fault, n)
        assert T.failures(new)


@pytest.mark.parametrize("fault", T.MODEL_FAULTS)
def test_each_model_fault_is_outside_a_named_bar(fault):
    args, (_, g_ref), (_, c0), _ = _model(False)
    _, bad = T.model_chain(*args, order=0, fault=fault)
    fails = T.failures(T.measure(bad, c0, g_ref, model=True), True)
    print(f"FAULT {fault}: outside {len(fails)} bar(s), first: {fails[:1]}")
    assert fails


# ---------------------------------------------------------------------------------------------------------------------
# the glue
@pytest.mark.parametrize("M", T.LIN_M)
def test_glue_chain_is_inside_the_gemm_bars(M):
    for cls in T.LIN_CLASSES:
        x, w, dy = T.linear_inputs(cls, M)
        rdx, rdw, db64 = T.linear_refs(x, w, dy)
        for order in (0, 1):
            got = T.glue_chain(x, w, dy, order)
            if cls == "gauss":
                GR.assert_pinned(got["dx"], rdx, T.LIN_N, f"glue dX gauss M={M} order {order}")
                GR.assert_pinned(got["dw"], rdw, T.pad64(M), f"glue dW gauss M={M} order {order}")
            else:
                assert torch.equal(got["dx"].double(), rdx.out) and torch.equal(got["dw"].double(), rdw.out), (cls, M, order)
            want, lo, hi = T.bias_grad_bound(dy)
            assert bool(((got["db"].double() >= lo) & (got["db"].double() <= hi)).all()), (cls, M)
        if cls == "selector":
            col = T.selector_col(M, T.LIN_N)
            assert torch.equal(got["dw"][col].double(), dy[torch.arange(M), col].double()[:, None] * x.double())
        # the two glue faults
        if M > 1:
            bad = T.glue_chain(x, w, dy, 0, "bias_drops_last_row")["db"].double()
            _, lo, hi = T.bias_grad_bound(dy)
            assert not bool(((bad >= lo) & (bad <= hi)).all()), (cls, M)
        if M % 64:
            assert bool(torch.isnan(T.glue_chain(x, w, dy, 0, "pad_row_garbage")["dw"].float()).any())


def test_loss_chain_and_unpatchify_backward():
    g = torch.Generator().manual_seed(3)
    pred, target = torch.randn((16, 3, 8, 12), generator=g).to(T.BF), torch.randn((16, 3, 8, 12), generator=g).to(T.BF)
    l1, d1 = T.loss_chain(pred, target, 0.37)
    lh, dh = T.loss_chain(pred, target, 0.37, 0.5)
    assert lh == 0.5 * l1 and torch.equal(dh.float(), d1.float() * 0.5)           # a power of two: exact
    _, d3 = T.loss_chain(pred, target, 0.37, 3.0)
    import backward_refs as BR
    import forward_refs as FR
    want = FR.rb(3.0 * BR.mse_ref(pred, target, 0.37)[1])
    assert int(FR.bf16_steps(d3, want.to(T.BF)).max()) <= 1
    dout = torch.randint(-8, 9, (16, 3, 8, 12), generator=g).double()
    tok = T.unpatchify_bwd_ref(dout, 16, 3, 4, 6)
    assert torch.equal(tok, dout.reshape(16, 3, 4, 2, 6, 2).permute(1, 2, 4, 3, 5, 0).reshape(72, 64))
