"""CPU evidence for tests/cross_fold_refs.py, the yardstick of tests/test_cross_fold_pinned_gpu.py: the fp64 references are what they
say, the RIGHT fp32 restatements of gf_cross_probs and gf_cross_fold_table are inside every bar on every input the GPU test runs, the
exact classes equal the restatements bit for bit, and each injected fault is outside a named bar.

What each fault measures on its case of FAULT_CASES (ratios of the allowance) and what the bars held before made of it — `old`: per
element 2^-8 + 1e-4 relative + 1e-7, last key + residue 2e-4 relative, row sum 2e-2 (the table: 2^-8 |ref| + 1e-6 and the column copy);
`rel-L2`: the folded product's whole-tensor error within 1.1 x the unfolded chain's, the only bar the product had:
    fault                      caught by (new)                                          old       rel-L2 (fault / unfolded)
    residue_dropped            last key 14 x, row sum 12 x (pad_dominant)               caught    PASSED  2.57e-3 / 2.47e-3
    residue_shifted            the same, and a non-zero pad column                      caught    PASSED  2.57e-3 / 2.47e-3
    mult_missing               element 2e4 x                                            caught    caught
    mult_on_wrong_key          element 323 x (m = 2)                                    caught    caught
    mask_drops_last            element 2.5e4 x                                          caught    caught
    mask_reads_one_past        element 122 x, row sum 216 x (far_below)                 caught    caught
    halves_swapped             element 1.7e7 x; one_hot: "expected column 0, found 32"  caught    caught
    d_groups_natural           element 1.0e7 x; one_hot: "expected column 4, found 16"  caught    caught
    max_first_half             one_hot: NaN wherever the hot key is >= 32; on std data  caught    caught
                               the fault is invisible to every bar, old and new (the
                               softmax is shift-invariant: asserted)
    norm_by_rounded_sum        differing bits 155 of 15 867 against a cap of 15; last   caught    PASSED  2.45e-3 / 2.37e-3
                               key 2.2 x (std1).  On pad_dominant the fault is no fault:
                               the dominant weight is exp2(0) = 1, which bf16 holds
    head_plus_one              element 3.8e5 x                                          caught    caught
    row_2pct                   element 5.1 x, last key 25 x, row sum 14 x (std3)        caught    caught  2.88e-3 / 2.32e-3 (1.24 x)
    table_col_zero             column n != column n - 1; 600 elements outside (b)       caught    caught  (1.20 x)
    table_col_from_n_minus_2   column n != column n - 1; worst 1.7e4 x of (b)           caught    caught  (1.27 x)
    table_bf16_partials        (a): 35 % of the bits differ; (b) worst 33 x             caught    caught  (1.38 x)
    table_head_slice_off       (b) worst 2e4 x                                          caught    caught
So the expectation that a 2 % row, the table's bf16 partial sums and the rounded row sum would pass the old bars held for none of
the three against the old per-element bars AT THESE CASES (what the old tests lacked was the cases, and for the table any bar beyond
one shape); against the rel-L2 bar, the only one the folded product had, the rounded row sum and the dropped residue pass.  Both sets
are asserted below (OLD_BARS_PASS, REL_L2_PASS), not assumed.  The last-key bar reaches at most 0.035 of its allowance on a right
restatement: E is a worst case over 128 roundings; what it misses at small relative errors the differing-bits bar sees.
"""
import pytest
import torch

import cross_fold_refs as R
import gemm_refs as G
from forward_refs import bits

TWIN = (129, 41, 3, 472.0)
# fault -> (class, q_len, n_keys, heads, m, the bar that must catch it)
FAULT_CASES = {
    "residue_dropped": ("pad_dominant", *TWIN, "last"),
    "residue_shifted": ("pad_dominant", *TWIN, "last"),
    "mult_missing": ("std1", *TWIN, "elem"),
    "mult_on_wrong_key": ("std1", 129, 41, 3, 2.0, "elem"),
    "mask_drops_last": ("std1", *TWIN, "elem"),
    "mask_reads_one_past": ("far_below", *TWIN, "elem"),
    "halves_swapped": ("std1", *TWIN, "elem"),
    "d_groups_natural": ("std1", *TWIN, "elem"),
    "max_first_half": ("one_hot", *TWIN, "elem"),
    "norm_by_rounded_sum": ("std1", *TWIN, "bits"),
    "head_plus_one": ("std1", *TWIN, "elem"),
    "row_2pct": ("std3", *TWIN, "elem"),
}
TABLE_FAULT_CASE = (41, 3, 200)                 # n_keys, heads, n_out (gauss)
# the faults the bars held before this file let through on the cases above (measured by test_old_bars_verdicts)
OLD_BARS_PASS = set()
REL_L2_PASS = {"residue_dropped", "residue_shifted", "norm_by_rounded_sum"}

_CACHE = {}


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _case(name, sq, n, n_pad, heads, m):
    key = (name, sq, n, n_pad, heads, m)
    if key not in _CACHE:
        _CACHE[key] = R.case(*key)
    return _CACHE[key]


def _fault_case(fault):
    name, sq, n, heads, m, bar = FAULT_CASES[fault]
    return _case(name, sq, n, R.pad_min(n), heads, m), bar


def _faulty(cs, fault):
    return R.probs_f32(cs.q, cs.k, cs.heads, cs.scale, cs.m, cs.n_pad, fault=fault)


def _table_operands(cs, n_out=256):
    v, w = R.table_inputs("gauss", cs.n, cs.heads, n_out)
    b = (0.1 * torch.randn(n_out, generator=torch.Generator().manual_seed(5))).to(R.BF)
    return v, w, b


# ---------------------------------------------------------------------------------------------------------------------
def test_references_are_what_they_say():
    cs = _case("std3", 33, 17, 32, 3, 5.0)
    kk = torch.cat([cs.k, cs.k[-1:].expand(4, -1)])                   # the multiplicity written out
    long = R.probs_ref(cs.q, kk, 3, cs.scale, 1.0)[0]
    assert float((cs.p[:, :, :-1] - long[:, :, :16]).abs().max()) < 1e-15
    assert float((cs.p[:, :, -1] - long[:, :, 16:].sum(-1)).abs().max()) < 1e-15 and float((cs.p.sum(-1) - 1).abs().max()) < 1e-14
    want = (cs.q.double()[7, 128:256] * cs.k.double()[3, 128:256]).abs().sum()
    assert abs(float(cs.S_abs[7, 1, 3] - want)) < 1e-12
    img = R.probs_layout(cs.p, 32)
    assert img.shape == (33, 3, 32) and not bool(img[:, :, 18:].any())
    pl = cs.p[:, :, -1]
    assert torch.equal(img[:, :, 17].double(), R.rb(pl - R.rb(pl))) and torch.equal(img[:, :, :17].double(), R.rb(cs.p))
    v, w = R.table_inputs("gauss", 17, 3, 65)
    r = R.table_ref(v, w, 3, 32)
    u = r.out.view(65, 3, 32)
    want = (v.double()[5, 256:384] * w.double()[60, 256:384]).sum()
    assert float((u[60, 2, 5] - want).abs()) <= 2.0 ** -8 * abs(float(want))
    assert torch.equal(u[:, :, 17], u[:, :, 16]) and not bool(u[:, :, 18:].any())


def test_bits_cap_is_gemm_refs_cap_and_holds_at_large_means():
    for n, p in ((15867, 1.26e-4), (4096, 2.0 ** -10), (63984, 4e-4), (1089, 2e-3)):
        assert R.bits_cap(n, p) == G.cap(n, p)
    big = R.bits_cap(63984, 1.3e-3)                       # mean 83: gemm_refs.cap's early stop returns 0 here
    assert G.cap(63984, 1.3e-3) == 0 and 83 + 5 * 83 ** 0.5 < big < 83 + 8 * 83 ** 0.5, big
    # the two computations agree where both are right (mean 25: the boundary's lower side, recomputed over the whole support)
    i = torch.arange(0, 25001, dtype=torch.float64)
    lp = torch.lgamma(torch.tensor(25001.0, dtype=torch.float64)) - torch.lgamma(i + 1) - torch.lgamma(25000 - i + 1) + i * torch.log(torch.tensor(1e-3, dtype=torch.float64)) \
        + (25000 - i) * torch.log1p(torch.tensor(-1e-3, dtype=torch.float64))
    upper = torch.flip(torch.cumsum(torch.flip(torch.exp(lp), [0]), 0), [0])
    assert int(torch.nonzero(upper[1:] < G.TAIL)[0]) == G.cap(25000, 1e-3)


def test_case_tables_cover_every_edge():
    assert {n for _, n, _ in R.PAIRS} == set(R.N_KEYS) | {5, 20} and {q for q, _, _ in R.PAIRS} == set(R.Q_LENS)
    for n, n_pad in R.KEY_CASES:
        assert len({q for q, nn, pp in R.PAIRS if (nn, pp) == (n, n_pad)}) >= 2, (n, n_pad)
    for q in R.Q_LENS:
        assert len({(n, p) for qq, n, p in R.PAIRS if qq == q}) >= 2, q
    assert all(n < p <= 64 and p % 16 == 0 for _, n, p in R.PAIRS)
    t = R.table_cases()
    assert len(set(t)) == len(t) == len(R.KEY_CASES) * len(R.N_OUT) * len(R.HEADS)


@pytest.mark.parametrize("sq,n,n_pad", R.PAIRS)
def test_right_probs_restatement_is_inside_every_bar_at_every_edge(sq, n, n_pad):
    """The inputs of test_probs_every_edge: the pair x heads x m on std1."""
    worst = dict(elem=0.0, last=0.0, row=0.0)
    for heads in R.HEADS:
        for m in R.MULTS:
            cs = _case("std1", sq, n, n_pad, heads, m)
            j = R.judge_probs(R.restated(cs), cs)
            assert not R.failed_bars(j), (heads, m, R.describe_probs(j))
            worst = {b: max(worst[b], j[b]) for b in worst}
    print(f"q={sq} keys={n} n_pad={n_pad}: the restatement's worst ratios {worst}")
    assert worst["elem"] <= 1.0 and worst["last"] <= 0.25 and worst["row"] <= 1.0


def test_right_probs_restatement_is_inside_every_bar_on_every_class():
    """The inputs of the GPU test's class, kernel-2, product and memory tests; the worst ratio of each bar is recorded: element 0.97 (one bf16 rounding at the bottom of
    a binade: the bar is u p and a rounding reaches it), last key + residue 0.03, row sum 0.54."""
    worst = dict(elem=0.0, last=0.0, row=0.0)
    for name, sq, n, n_pad, heads, m in R.other_probs_cases():
        cs = _case(name, sq, n, n_pad, heads, m)
        j = R.judge_probs(R.restated(cs), cs)
        print(f"{name} q={sq} keys={n} n_pad={n_pad} heads={heads} m={m}: {R.describe_probs(j)}")
        assert not R.failed_bars(j), (name, R.describe_probs(j))
        worst = {b: max(worst[b], j[b]) for b in worst}
    print(f"worst over the classes: {worst}")
    assert 0.9 < worst["elem"] <= 1.0 and worst["last"] <= 0.05 and worst["row"] <= 0.6


def test_exact_classes_equal_the_restatement_bit_for_bit():
    for sq, n, n_pad in R.PAIRS:
        for heads in R.HEADS if n in R.UNIFORM_N else ():
            cs = _case("uniform", sq, n, n_pad, heads, 1.0)
            want = R.probs_layout(cs.p, cs.n_pad)
            assert torch.equal(want[:, :, :n].float(), torch.full((sq, heads, n), 1.0 / n)) and not bool(want[:, :, n:].any())
            assert torch.equal(bits(R.restated(cs)), bits(want)), n
        for m in R.MULTS:
            cs = _case("one_hot", sq, n, n_pad, 3, m)
            assert R.one_hot_report(R.restated(cs), cs) is None, R.one_hot_report(R.restated(cs), cs)
            hot = R.hot_key(torch.arange(sq)[:, None], torch.arange(3)[None, :], n)
            assert torch.equal(R.restated(cs).float().argmax(-1), hot) and float(R.restated(cs).float().sum()) == sq * 3
    for name in ("integers", "selector"):
        for n, n_pad, n_out, heads in R.table_cases():
            v, w = R.table_inputs(name, n, heads, n_out)
            r = R.table_ref(v, w, heads, n_pad)
            acc = R.table_sums(v, w, heads)[0]
            assert torch.equal(R.rb(acc), acc), f"{name}: a table entry is not exactly representable"
            assert torch.equal(bits(R.table_f32(v, w, heads, n_pad)), bits(r.out)), (name, n, n_out, heads)
            if name == "selector":
                rows = torch.arange(n_out)
                for h in range(heads):
                    d = R.selector_d(rows, h)
                    want = v.double()[:, h * 128 + d].T * w.double()[rows, h * 128 + d][:, None]
                    assert torch.equal(r.out.view(n_out, heads, n_pad)[:, h, :n], want), (n, h)


def test_right_table_restatement_is_inside_both_bars():
    worst, share = 0.0, 0.0
    for n, n_pad, n_out, heads in R.table_cases() + [(n, p, o, h) for n, p, h, o in R.MEM_TABLE]:
        v, w = R.table_inputs("gauss", n, heads, n_out)
        j = G.judge(R.table_f32(v, w, heads, n_pad), R.table_ref(v, w, heads, n_pad), 128)
        assert all(G.passes(j)), (n, n_out, heads, G.describe(j))
        worst, share = max(worst, j["worst"]), max(share, j["share"])
    print(f"table restatement: worst ratio of bar (b) {worst:.3f}, worst differing share {share:.2e}")
    assert worst <= 1.0 and share <= G.SHARE_CAP


def test_right_folded_product_is_inside_its_bound():
    for name, sq, n, heads, m in R.PRODUCT_CASES:
        cs = _case(name, sq, n, R.pad_min(n), heads, m)
        v, w, b = _table_operands(cs)
        F, bound = R.product_ref(cs, v, w, b)
        hat = R.product_hat(R.restated(cs).view(sq, -1), R.table_f32(v, w, heads, cs.n_pad), b)
        ratio = float(((hat - F).abs() / bound).max())
        print(f"folded product {name} q={sq} keys={n}: worst {ratio:.3f} of the bound")
        assert ratio <= 1.0


@pytest.mark.parametrize("fault", R.PROBS_FAULTS)
def test_every_probs_fault_is_outside_its_named_bar(fault):
    cs, bar = _fault_case(fault)
    j = R.judge_probs(_faulty(cs, fault), cs)
    print(f"{fault} on {cs.name}: outside {R.failed_bars(j)}; {R.describe_probs(j)}")
    assert bar in R.failed_bars(j), (fault, bar, R.describe_probs(j))
    if fault in ("halves_swapped", "d_groups_natural", "max_first_half"):      # the class that names the columns
        oh = _case("one_hot", 129, 41, 48, 3, 472.0)
        msg = R.one_hot_report(_faulty(oh, fault), oh)
        print(msg)
        assert msg is not None and "expected 1.0 in column" in msg
    if fault == "residue_shifted":
        assert "zeros" in R.failed_bars(j)
    if fault == "max_first_half":                                               # invisible on shift-invariant data, to any bar
        std = _case("std1", *TWIN[:2], 48, *TWIN[2:])
        assert not R.failed_bars(R.judge_probs(_faulty(std, fault), std))


def _table_figures(fault):
    n, heads, n_out = TABLE_FAULT_CASE
    n_pad = R.pad_min(n)
    v, w = R.table_inputs("gauss", n, heads, n_out)
    r = R.table_ref(v, w, heads, n_pad)
    got = R.table_f32(v, w, heads, n_pad, fault=fault)
    g3, r3 = got.view(n_out, heads, n_pad), r.out.view(n_out, heads, n_pad)
    copy_ok = torch.equal(g3[:, :, n], g3[:, :, n - 1]) and not bool(g3[:, :, n + 1:].any())
    old = copy_ok and bool(((g3[:, :, :n].double() - r3[:, :, :n]).abs() <= r3[:, :, :n].abs() * 2.0 ** -8 + 1e-6).all())
    return G.judge(got, r, 128), copy_ok, old, (v, w, got)


@pytest.mark.parametrize("fault", R.TABLE_FAULTS)
def test_every_table_fault_is_outside_a_bar(fault):
    j, copy_ok, _, _ = _table_figures(fault)
    a, b = G.passes(j)
    print(f"{fault}: {G.describe(j)}; column n_keys == column n_keys - 1 and zero pad: {copy_ok}")
    if fault in ("table_col_zero", "table_col_from_n_minus_2"):
        assert not copy_ok and not b
    elif fault == "table_bf16_partials":
        assert not a and j["share"] > 0.1, "bar (a) names the second rounding"
    else:
        assert not b and j["worst"] > 100


def _rel_l2_verdict(cs, p_hat, u_hat, v, w, b):
    """The old whole-tensor bar: the folded product (one bf16 rounding, as the GEMM's) within 1.1 x the unfolded chain's rel-L2."""
    F, _ = R.product_ref(cs, v, w, b)
    e_fold = float((R.rb(R.product_hat(p_hat, u_hat, b)) - F).norm() / F.norm())
    e_plain = float((R.unfolded_chain(cs, v, w, b) - F).norm() / F.norm())
    return e_fold <= 1.1 * e_plain, e_fold, e_plain


def test_old_bars_verdicts():
    """Which faults the bars held before let through — measured here, asserted against OLD_BARS_PASS and REL_L2_PASS."""
    passed, passed_l2 = set(), set()
    for fault in R.PROBS_FAULTS:
        cs, _ = _fault_case(fault)
        got = _faulty(cs, fault)
        v, w, b = _table_operands(cs)
        ok_l2, e_fold, e_plain = _rel_l2_verdict(cs, got.view(got.shape[0], -1), R.table_f32(v, w, cs.heads, cs.n_pad), v, w, b)
        ok_elem = R.old_probs_bars(got, cs)
        print(f"{fault}: old per-element / last-key / row-sum bars {'PASS' if ok_elem else 'catch'}; rel-L2 {e_fold:.3e} against "
              f"{e_plain:.3e} unfolded: {'PASS' if ok_l2 else 'catch'}")
        passed |= {fault} if ok_elem else set()
        passed_l2 |= {fault} if ok_l2 else set()
    cs = _case("std3", *TWIN[:2], 48, *TWIN[2:])
    for fault in R.TABLE_FAULTS:
        _, _, old, (v, w, got) = _table_figures(fault)
        b = torch.zeros(got.shape[0], dtype=R.BF)
        ok_l2, e_fold, e_plain = _rel_l2_verdict(cs, R.restated(cs).view(129, -1), got, v, w, b)
        print(f"{fault}: old table bar {'PASS' if old else 'catch'}; rel-L2 {e_fold:.3e} against {e_plain:.3e}: {'PASS' if ok_l2 else 'catch'}")
        passed |= {fault} if old else set()
        passed_l2 |= {fault} if ok_l2 else set()
    assert passed == OLD_BARS_PASS and passed_l2 == REL_L2_PASS, (passed, passed_l2)
