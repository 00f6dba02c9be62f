"""gf_lora_grad without a GPU: the declarations and the binding, the slab rule (the library's host functions against
tests/lora_train_refs.py's restatement of it), the wrapper's device-free refusals, and the sensitivity of what
tests/test_lora_grad_gpu.py holds the kernel to: the fp32 restatement in the kernel's slab order passes gemm_refs' two bars on
every gauss input of the GPU test and equals the chain on the exact classes; each stated fault is outside a bar or breaks an exact
class."""
import pytest
import torch

import gemm_refs as G
import lora_train_refs as T
from forward_refs import bits

BF = torch.bfloat16
CASES = T.grad_cases()


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI
def test_the_declarations_and_the_revision():
    import ctypes
    from goal_force_amd import _lib
    v, i64, f, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int
    assert _lib.ABI_VERSION == 20
    for name in ("gf_lora_grad_slabs", "gf_lora_grad_slab_rows", "gf_lora_grad_workspace_bytes"):
        assert _lib.BINDINGS[name] == (i64, [i64, i64, i64])
    assert _lib.BINDINGS["gf_lora_grad"] == (i, [v, i64, v, i64, v, i64, i64, i64, i64, f, i, v, v])
    lib = _lib.load()
    assert lib.gf_abi_version() == 20


def test_the_slab_rule_is_the_librarys_and_fills_the_device_at_the_production_shapes():
    from goal_force_amd import _lib
    lib = _lib.load()
    shapes = [(M, C) for M in (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 769, 1024, 4097, 32760) for C in (8, 64, 72, 520, 5120, 13824)]
    shapes += [(M, C) for M, C, *_ in CASES]
    for M, C in shapes:
        n, rows = T.slab_plan(M, C)
        for rp in (32, 256):
            assert (lib.gf_lora_grad_slabs(M, C, rp), lib.gf_lora_grad_slab_rows(M, C, rp)) == (n, rows), (M, C, rp)
            assert lib.gf_lora_grad_workspace_bytes(M, C, rp) == T.workspace_bytes(M, C, rp)
        b = T.slab_bounds(M, C)
        assert [x for x, _ in b] == [s * rows for s in range(n)] and (not b or b[-1][1] == M) and all(e > s for s, e in b)
        assert all(e == b[i + 1][0] for i, (_, e) in enumerate(b[:-1])), "every token in exactly one slab"
        assert rows % T.TOKEN_TILE == 0 and n <= max(1, -(-M // (T.MIN_TILES * T.TOKEN_TILE)))
    for C in (5120, 13824):                       # the expert's widths at the training sequence: at least 4 workgroups per CU of 256
        n, _ = T.slab_plan(32760, C)
        assert 1024 <= n * -(-C // 64) <= 1024 + 256
    assert T.slab_plan(512, 5120)[0] == 2         # cross-attention k / v: the context rows
    # a shape the entry refuses has no plan
    for M, C, rp in ((-1, 64, 32), (64, 60, 32), (64, 0, 32), (64, 64, 0), (64, 64, 48), (64, 64, 288), (1 << 30, 64, 32)):
        assert lib.gf_lora_grad_slabs(M, C, rp) == lib.gf_lora_grad_slab_rows(M, C, rp) == lib.gf_lora_grad_workspace_bytes(M, C, rp) == 0
    assert len(T.slab_bounds(T.two_slab_m(T.SLAB_C), T.SLAB_C)) == 2 and len(T.slab_bounds(T.two_slab_m(T.SLAB_C) - 1, T.SLAB_C)) == 1
    last = T.slab_bounds(T.one_row_last_slab_m(T.SLAB_C), T.SLAB_C)
    assert len(last) >= 3 and last[-1][1] - last[-1][0] == 1


def test_the_cases_cover_every_axis_value():
    assert {c[0] for c in CASES} >= set(T.GRAD_M) and {c[1] for c in CASES} >= set(T.GRAD_C)
    assert {(c[2], c[3]) for c in CASES} >= set(T.GRAD_RANKS) and {c[4] for c in CASES} == set(T.SCALES) and {c[5] for c in CASES} == {False, True}
    assert {c[2] for c in CASES} == {32, 64, 256} and {c[3] for c in CASES} == {1, 4, 33}


def test_wrapper_refusals_that_need_no_device():
    from goal_force_amd import ops
    from goal_force_amd._lib import GoalForceError
    y, t = torch.zeros((4, 16), dtype=BF), torch.zeros((4, 32), dtype=BF)
    with pytest.raises(GoalForceError, match=r"lora_grad\.y: tensor must be on the GPU"):
        ops.lora_grad(y, t, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# the bars: the restatement passes, the faults do not
def _case(cls, case):
    M, C, rp, r, scale, tr = case
    return T.grad_inputs(cls, M, C, rp, r, scale, tr)


def _restate(d, **kw):
    return T.grad_restate(d["Y"], d["T"], d["scale"], d["transposed"], rank=d["rank"], **kw)


def test_restatement_passes_both_bars_on_every_gauss_input_and_equals_the_chain_on_the_exact_classes():
    worst = (0.0, 0.0)
    for case in CASES:
        d = _case("gauss", case)
        ref = T.grad_ref(d)
        for tile in (32, 64):
            j = G.judge(_restate(d, tile=tile), ref, case[0])
            assert G.passes(j) == (True, True), (case, G.describe(j))
            worst = (max(worst[0], j["share"]), max(worst[1], j["worst"]))
        for cls in ("selector", "integers"):
            d = _case(cls, case)
            assert torch.equal(bits(_restate(d)), bits(T.grad_ref(d).out.to(BF))), (cls, case)
    print(f"lora_grad restatement: worst differing share {worst[0]:.2e}, worst ratio of (b) {worst[1]:.2f}")


def test_exact_classes_pad_columns_and_zero_scale_are_plus_zero():
    for case in CASES:
        for cls in T.CLASSES:
            d = _case(cls, case)
            out = T.grad_ref(d).out.to(BF)
            pad = out[d["rank"]:] if d["transposed"] else out[:, d["rank"]:]
            assert not bool(bits(pad).any()), "the rank's padding is +0 bit for bit"
            if d["scale"] == 0.0:
                assert not bool(bits(out).any())
            elif case[0] > 1:
                assert bool(out.any())


def _caught(fault, case):
    """Does any of the three classes see the fault at this case?"""
    for cls in T.CLASSES:
        d = _case(cls, case)
        got, ref = _restate(d, fault=fault), T.grad_ref(d)
        if cls == "gauss":
            a, b = G.passes(G.judge(got, ref, case[0]))
            if not (a and b):
                return True
        elif not torch.equal(bits(got), bits(ref.out.to(BF))):
            return True
    return False


@pytest.mark.parametrize("fault", T.GRAD_FAULTS)
def test_each_fault_is_outside_a_bar_or_breaks_an_exact_class(fault):
    seen = 0
    for case in CASES:
        M, C, rp, r, scale, tr = case
        slabs = T.slab_plan(M, C)[0]
        if scale == 0.0:
            continue                    # (every fault of the sum is multiplied away)
        if fault == "scale_twice" and scale == 1.0:
            continue
        if fault == "partial_bf16" and scale == 1.0 and slabs == 1:
            continue                    # (one slab at scale 1: the partial's rounding IS the chain's)
        assert _caught(fault, case), f"{fault} passes at {case}"
        seen += 1
    assert seen >= 6
