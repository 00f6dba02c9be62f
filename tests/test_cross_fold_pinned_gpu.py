"""The folded cross-attention (goal_force_amd/csrc/gf_cross_fold.hip: gf_cross_probs, gf_cross_fold_table) pinned element
by element against the fp64 references of tests/cross_fold_refs.py, through the raw C ABI so that n_pad, strides, alignment and the
refusals are reachable.

P is held to the five bars of the helper's docstring (element, last key + residue, row sum, zero pad columns, differing bits against
twice the fp32 restatement's share), U to bits on the exact classes and to gemm_refs' two bars on Gaussians, the folded product to its
own per-element bound and — through ops.gemm — to the pinned GEMM's chain.  tests/test_cross_fold_refs_cpu.py shows on the CPU that
the right restatements pass all of it and which injected faults do not.  Each comparison prints what it measured (`pytest -s`).

Edges: the `halves` switch at 32 -> 33 keys (at 32 keys the second MFMA half is skipped and the residue column lives in it), the
n_pad steps at 15 -> 16, 31 -> 32, 47 -> 48, n_pad above the minimum, the 32-row wave and 128-row workgroup of gf_cross_probs, the
64-row workgroup of gf_cross_fold_table, multiplicities 1, 2, 1.5, 472, 511.
"""
import pytest
import torch

import attention_fwd_refs as A
import cross_fold_refs as R
import gemm_refs as G

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HD = R.HD
SENT = 0x5A5A                       # a finite bf16 bit pattern (1.5e16) no output here comes near
GF_ERR_INVALID_ARG, GF_ERR_UNSUPPORTED = -1, -2
SIG = {
    "gf_cross_probs": "q k p q_len n_keys n_pad heads head_dim q_stride k_stride p_stride scale mult stream",
    "gf_cross_fold_table": "v w u n_keys n_pad heads head_dim n_out v_stride w_stride u_stride stream",
    "gf_flash_attn_fwd_lastmult": "q k v o q_len n_keys heads head_dim q_stride k_stride v_stride o_stride scale mult stream",
}
POINTERS = ("q", "k", "p", "v", "w", "u", "o")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from goal_force_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    return ops._lib.load()


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


_CACHE = {}


def _case(name, sq, n, n_pad, heads, m):
    """A probs case (inputs, fp64 reference, bounds): computed once and left unchanged."""
    key = (name, sq, n, n_pad, heads, m)
    if key not in _CACHE:
        _CACHE[key] = R.case(*key)
    return _CACHE[key]


def _raw(lib, entry, a, over=None):
    a = dict(a)
    a.update(over or {})
    assert set(over or {}) <= set(SIG[entry].split()), (entry, over)
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())          # noqa: E731
    rc = getattr(lib, entry)(*[ptr(a[n]) if n in POINTERS else a[n] for n in SIG[entry].split()])
    torch.cuda.synchronize()
    return rc


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sentinel(rows, cols):
    buf = torch.empty((rows, cols), dtype=BF, device="cuda")
    buf.view(torch.int16).fill_(SENT)
    return buf


def _probs_args(q, k, p, cs, **more):
    a = dict(q=q, k=k, p=p, q_len=q.shape[0], n_keys=k.shape[0], n_pad=cs.n_pad, heads=cs.heads, head_dim=HD, q_stride=q.stride(0),
             k_stride=k.stride(0), p_stride=p.stride(0), scale=float(cs.scale), mult=float(cs.m), stream=_stream())
    a.update(more)
    return a


def _probs(lib, cs):
    """gf_cross_probs on the case's contiguous operands -> [Sq, H, n_pad] bf16 on the CPU; every element was written."""
    sq = cs.q.shape[0]
    p = _sentinel(sq, cs.heads * cs.n_pad)
    assert _raw(lib, "gf_cross_probs", _probs_args(cs.q.cuda(), cs.k.cuda(), p, cs)) == 0, lib.gf_last_error().decode()
    assert not bool((p.view(torch.int16) == SENT).any()), "an element of P was not written"
    return p.cpu().view(sq, cs.heads, cs.n_pad)


def _table_args(v, w, u, n_pad, heads, **more):
    a = dict(v=v, w=w, u=u, n_keys=v.shape[0], n_pad=n_pad, heads=heads, head_dim=HD, n_out=w.shape[0], v_stride=v.stride(0),
             w_stride=w.stride(0), u_stride=u.stride(0), stream=_stream())
    a.update(more)
    return a


def _table(lib, v, w, heads, n_pad):
    u = _sentinel(w.shape[0], heads * n_pad)
    assert _raw(lib, "gf_cross_fold_table", _table_args(v.cuda(), w.cuda(), u, n_pad, heads)) == 0, lib.gf_last_error().decode()
    assert not bool((u.view(torch.int16) == SENT).any()), "an element of U was not written"
    return u


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------------
# gf_cross_probs
@pytest.mark.parametrize("sq,n,n_pad", R.PAIRS)
def test_probs_every_edge(lib, sq, n, n_pad):
    """The covering pair x heads 1 / 3 / 8 x m on std1 through all bars; one_hot at the pair (every m: the hot weight is exactly 1 on
    the last key and off it, every other exactly 0, the residue 0 but for a hot last key at m != 1: cross_fold_refs.one_hot_report) and uniform where n_keys is a power of two, bit for bit."""
    worst = dict(elem=0.0, last=0.0, row=0.0, share=0.0, rate=0.0)
    for heads in R.HEADS:
        for m in R.MULTS:
            cs = _case("std1", sq, n, n_pad, heads, m)
            j = R.assert_probs(_probs(lib, cs), cs, f"std1 q={sq} keys={n} n_pad={n_pad} heads={heads} m={m}")
            worst = {b: max(worst[b], j[b]) for b in worst}
    print(f"EDGE q={sq} keys={n} n_pad={n_pad}: worst element {worst['elem']:.3f}, last key {worst['last']:.3f}, row sum {worst['row']:.3f}; "
          f"worst differing share {worst['share']:.2e} (restatement's worst {worst['rate']:.2e})")
    for m in R.MULTS:
        cs = _case("one_hot", sq, n, n_pad, 3, m)
        msg = R.one_hot_report(_probs(lib, cs), cs)
        assert msg is None, msg
    if n in R.UNIFORM_N:
        for heads in R.HEADS:
            cs = _case("uniform", sq, n, n_pad, heads, 1.0)
            got = _probs(lib, cs)
            assert _same(got, R.probs_layout(cs.p, n_pad)), f"uniform q={sq} keys={n} heads={heads}: not 1/{n} in every live column, 0 after"


@pytest.mark.parametrize("name", R.CLASSES)
def test_probs_data_classes(lib, name):
    """Every class at the production shape's small twin (129 queries, 41 keys, 3 heads, m 472) and at 33 x 33 keys, 1 head."""
    for sq, n, heads, m in R.CLASS_SHAPES:
        cs = _case(name, sq, n, R.pad_min(n), heads, m)
        R.assert_probs(_probs(lib, cs), cs, f"CLASS {name} q={sq} keys={n} heads={heads} m={m}")


@pytest.mark.parametrize("name,sq,n,heads,m", R.K2_CASES)
def test_probs_agrees_with_kernel_2(lib, name, sq, n, heads, m):
    """P^ (the last key's weight with its residue) times V in fp64 against gf_flash_attn_fwd_lastmult's O on the same operands: the header
    promises the same fp32 score arithmetic.  Both are held to the same fp64 attention, so the distance is within kernel 2's bound
    (attention_fwd_refs) plus P's own: sum_j (u p_j + p_j E_j + floor) |V_jd|, the last key's term with 2^-16 for u."""
    cs = _case(name, sq, n, R.pad_min(n), heads, float(m))
    got = _probs(lib, cs).double()
    v = torch.randn((n, heads * HD), generator=torch.Generator().manual_seed(n)).to(BF)
    o = _sentinel(sq, heads * HD)
    q, k, vd = cs.q.cuda(), cs.k.cuda(), v.cuda()
    a = dict(q=q, k=k, v=vd, o=o, q_len=sq, n_keys=n, heads=heads, head_dim=HD, q_stride=q.stride(0), k_stride=k.stride(0), v_stride=vd.stride(0),
             o_stride=o.stride(0), scale=float(cs.scale), mult=float(m), stream=_stream())
    assert _raw(lib, "gf_flash_attn_fwd_lastmult", a) == 0, lib.gf_last_error().decode()
    ref = A.attn_ref(cs.q, cs.k, v, heads, cs.scale, mult=m)
    assert float((ref.P.transpose(0, 1) - cs.p).abs().max()) < 1e-13, "the two fp64 references disagree"
    pt = got[:, :, :n].clone()
    pt[:, :, n - 1] += got[:, :, n]
    V = v.double().view(n, heads, HD)
    o_hat = torch.einsum("shj,jhd->shd", pt, V).reshape(sq, -1)
    pb = cs.elem.clone()
    pb[:, :, -1] = cs.last
    allow = A.bounds(ref, "k2")[0] + torch.einsum("shj,jhd->shd", pb, V.abs()).reshape(sq, -1)
    err = (o_hat - o.cpu().double()).abs()
    print(f"K2 {name} q={sq} keys={n} heads={heads} m={m}: P^ V against kernel 2's O: worst {float((err / allow).max()):.3f} of the allowance; "
          f"P^ V against fp64: {A.rel_l2(o_hat, ref.o):.2e}, kernel 2: {A.rel_l2(o.cpu(), ref.o):.2e} rel-L2")
    assert bool((err <= allow).all()), float((err / allow).max())


# ---------------------------------------------------------------------------------------------------------------------
# gf_cross_fold_table
@pytest.mark.parametrize("n,n_pad", R.KEY_CASES)
def test_table_every_edge(lib, n, n_pad):
    """Every n_out x heads at this key case: integers and selector bit for bit, gauss through gemm_refs' two bars (K = 128); column
    n_keys equal to column n_keys - 1 and the later columns +0 bit for bit."""
    worst, share = 0.0, 0.0
    for _, _, n_out, heads in [c for c in R.table_cases() if c[:2] == (n, n_pad)]:
        for name in R.TABLE_CLASSES:
            v, w = R.table_inputs(name, n, heads, n_out)
            r = R.table_ref(v, w, heads, n_pad)
            u = _table(lib, v, w, heads, n_pad).cpu()
            u3 = u.view(n_out, heads, n_pad)
            what = f"TABLE {name} keys={n} n_pad={n_pad} n_out={n_out} heads={heads}"
            assert _same(u3[:, :, n], u3[:, :, n - 1]), f"{what}: column n_keys is not column n_keys - 1"
            assert bool((u3[:, :, n + 1:].contiguous().view(torch.int16) == 0).all()), f"{what}: a pad column is not +0"
            if name == "gauss":
                j = G.judge(u, r, HD)
                assert all(G.passes(j)), f"{what}: {G.describe(j)}; first (row, column): {j['first']}"
                worst, share = max(worst, j["worst"]), max(share, j["share"])
            elif not torch.equal(u.double(), r.out):
                row, col = (int(x) for x in torch.nonzero(u.double() != r.out)[0])
                h, j_ = divmod(col, n_pad)
                d = f", d = {int(R.selector_d(row, h))}" if name == "selector" else ""
                raise AssertionError(f"{what}: U[{row}, head {h}, j = {j_}{d}] is {float(u[row, col])}, exactly {float(r.out[row, col])} expected")
    print(f"TABLE keys={n} n_pad={n_pad}: gauss worst {worst:.3f} of bar (b), worst differing share {share:.2e}; integers and selector exact")


# ---------------------------------------------------------------------------------------------------------------------
# the folded product
@pytest.mark.parametrize("name,sq,n,heads,m", R.PRODUCT_CASES)
def test_folded_product_per_element(ops, lib, name, sq, n, heads, m):
    """P^ U^^T + b formed in fp64 from the device's own P^ and U^ against the unfolded fp64 function, per element (the fold's own error,
    apart from the GEMM's); then ops.gemm(P^, U^, b) through gemm_refs.assert_pinned against the chain on P^, U^ (K = 8 x 48 = 384)."""
    n_pad = R.pad_min(n)
    cs = _case(name, sq, n, n_pad, heads, m)
    D = heads * HD
    v, w = R.table_inputs("gauss", n, heads, D)
    b = (0.1 * torch.randn(D, generator=torch.Generator().manual_seed(5))).to(BF)
    p_hat = _probs(lib, cs)
    R.assert_probs(p_hat, cs, f"PRODUCT {name} q={sq} keys={n}")
    u_hat = _table(lib, v, w, heads, n_pad)
    F, bound = R.product_ref(cs, v, w, b)
    err = (R.product_hat(p_hat.view(sq, -1), u_hat.cpu(), b) - F).abs()
    print(f"PRODUCT {name} q={sq} keys={n} heads={heads}: fp64 product of P^, U^ against the unfolded function: worst {float((err / bound).max()):.3f} "
          f"of the bound, rel-L2 {float(err.norm() / F.norm()):.2e}")
    assert bool((err <= bound).all()), float((err / bound).max())
    pd = p_hat.view(sq, -1).cuda()
    got = ops.gemm(pd, u_hat, b.cuda())
    acc, S = G.product(pd.cpu(), u_hat.cpu())
    G.assert_pinned(got.cpu(), G.Ref(*G.chain(acc, b, G.EPI_BIAS, None, None, None, S), None, None), heads * n_pad, f"PRODUCT gemm {name} q={sq} keys={n}")


# ---------------------------------------------------------------------------------------------------------------------
# memory discipline
@pytest.mark.parametrize("sq,n,n_pad,heads", R.MEM_PROBS)
def test_memory_discipline_probs(lib, sq, n, n_pad, heads):
    """q and k are strided views of NaN-filled parents (stride heads*128 + 8, columns on both sides, rows behind), p goes into a
    sentinel-filled buffer with p_stride = heads*n_pad + 4: the same bits as the contiguous call, the gap, the rows >= q_len and the
    tail intact; q_len = 0 returns OK and writes nothing."""
    cs = _case("std1", sq, n, n_pad, heads, 472.0)
    want = _probs(lib, cs)
    R.assert_probs(want, cs, f"MEMORY q={sq} keys={n} n_pad={n_pad} heads={heads} (contiguous)")
    D, W = heads * HD, heads * n_pad
    q, k = (A.embed(t.cuda(), 5, 8, 0) for t in (cs.q, cs.k))
    assert all(t.stride(0) == D + 8 and t.data_ptr() % 16 == 0 and not t.is_contiguous() for t in (q, k))
    pbuf = _sentinel(sq + 3, W + 4)
    a = _probs_args(q, k, pbuf[:sq, :W], cs)
    assert a["p_stride"] == W + 4
    assert _raw(lib, "gf_cross_probs", a, dict(q_len=0)) == 0, lib.gf_last_error().decode()
    assert bool((pbuf.view(torch.int16) == SENT).all()), "q_len == 0 wrote something"
    assert _raw(lib, "gf_cross_probs", a) == 0, lib.gf_last_error().decode()
    pb = pbuf.view(torch.int16)
    assert bool((pb[:sq, W:] == SENT).all()), "the gap between two rows of P was written"
    assert bool((pb[sq:] == SENT).all()), "rows >= q_len were written"
    assert _same(pbuf[:sq, :W].cpu().view(sq, heads, n_pad), want), "P changed inside NaN surroundings / with a p_stride gap"


@pytest.mark.parametrize("n,n_pad,heads,n_out", R.MEM_TABLE)
def test_memory_discipline_table(lib, n, n_pad, heads, n_out):
    """v and w_o in NaN parents, u_stride = heads*n_pad + 3 and u at a 2-byte offset inside a sentinel-filled buffer: the same bits as the
    contiguous call, every guard element intact."""
    v, w = R.table_inputs("gauss", n, heads, n_out)
    want = _table(lib, v, w, heads, n_pad).cpu()
    W = heads * n_pad
    vs, ws = (A.embed(t.cuda(), 5, 8, 8) for t in (v, w))
    flat = _sentinel(1, 1 + (n_out + 2) * (W + 3)).view(-1)
    u = flat[1:1 + n_out * (W + 3)].view(n_out, W + 3)[:, :W]
    assert u.data_ptr() % 4 == 2 and u.stride(0) == W + 3
    assert _raw(lib, "gf_cross_fold_table", _table_args(vs, ws, u, n_pad, heads)) == 0, lib.gf_last_error().decode()
    fi = flat.view(torch.int16)
    assert int(fi[0]) == SENT and bool((fi[1 + n_out * (W + 3):] == SENT).all()), "an element before or behind U was written"
    assert bool((fi[1:1 + n_out * (W + 3)].view(n_out, W + 3)[:, W:] == SENT).all()), "the gap between two rows of U was written"
    assert _same(u.cpu(), want), "U changed inside NaN surroundings / at a 2-byte offset with a u_stride gap"


# ---------------------------------------------------------------------------------------------------------------------
# refusals
def _refusals(entry, heads, n, n_pad):
    D, W, bad = heads * HD, heads * n_pad, GF_ERR_INVALID_ARG
    keys = f"{entry}: 1 <= n_keys="
    out = {
        "head_dim_64": (dict(head_dim=64), GF_ERR_UNSUPPORTED, f"{entry}: head_dim=64 unsupported"),
        "heads_0": (dict(heads=0), bad, f"{entry}: bad sizes"), "heads_65536": (dict(heads=65536), bad, f"{entry}: bad sizes"),
        "n_keys_0": (dict(n_keys=0), bad, keys), "n_keys_64": (dict(n_keys=64, n_pad=64), bad, keys), "n_pad_8": (dict(n_pad=8), bad, keys),
        "n_pad_40": (dict(n_pad=40), bad, keys), "n_pad_80": (dict(n_pad=80), bad, keys), "n_pad_is_n_keys": (dict(n_keys=16, n_pad=16), bad, keys),
    }
    if entry == "gf_cross_probs":
        strides = f"{entry}: strides must cover the rows"
        out.update({
            "null_q": (dict(q=None), bad, f"{entry}: null pointer"), "null_k": (dict(k=None), bad, f"{entry}: null pointer"),
            "null_p": (dict(p=None), bad, f"{entry}: null pointer"), "q_len_negative": (dict(q_len=-1), bad, f"{entry}: bad sizes"),
            "q_len_2_30": (dict(q_len=1 << 30), bad, f"{entry}: bad sizes"),
            "q_stride_not_x8": (dict(q_stride=D + 4), bad, strides), "q_stride_short": (dict(q_stride=D - 8), bad, strides),
            "k_stride_not_x8": (dict(k_stride=D + 4), bad, strides), "k_stride_short": (dict(k_stride=D - 8), bad, strides),
            "p_stride_not_x4": (dict(p_stride=W + 2), bad, strides), "p_stride_short": (dict(p_stride=W - 4), bad, strides),
            "q_off_by_8_bytes": ("q+8", bad, f"{entry}: alignment"), "k_off_by_8_bytes": ("k+8", bad, f"{entry}: alignment"),
            "p_off_by_4_bytes": ("p+4", bad, f"{entry}: alignment"),
            "scale_0": (dict(scale=0.0), bad, f"{entry}: scale > 0"), "scale_negative": (dict(scale=-1.0), bad, f"{entry}: scale > 0"),
            "scale_nan": (dict(scale=float("nan")), bad, f"{entry}: scale > 0"),
            "multiplicity_below_1": (dict(mult=0.5), bad, f"{entry}: scale > 0, multiplicity >= 1"),
            "multiplicity_nan": (dict(mult=float("nan")), bad, f"{entry}: scale > 0, multiplicity >= 1"),
        })
    else:
        strides = f"{entry}: strides must cover the rows"
        out.update({
            "null_v": (dict(v=None), bad, f"{entry}: null pointer"), "null_w": (dict(w=None), bad, f"{entry}: null pointer"),
            "null_u": (dict(u=None), bad, f"{entry}: null pointer"), "n_out_0": (dict(n_out=0), bad, f"{entry}: bad sizes"),
            "n_out_2_30": (dict(n_out=1 << 30), bad, f"{entry}: bad sizes"),
            "v_stride_not_x8": (dict(v_stride=D + 4), bad, strides), "v_stride_short": (dict(v_stride=D - 8), bad, strides),
            "w_stride_not_x8": (dict(w_stride=D + 4), bad, strides), "w_stride_short": (dict(w_stride=D - 8), bad, strides),
            "u_stride_short": (dict(u_stride=W - 1), bad, strides),
            "v_off_by_8_bytes": ("v+8", bad, f"{entry}: alignment"), "w_off_by_8_bytes": ("w+8", bad, f"{entry}: alignment"),
            "u_off_by_1_byte": ("u+1", bad, f"{entry}: alignment"),
        })
    return out


@pytest.mark.parametrize("entry", ["gf_cross_probs", "gf_cross_fold_table"])
def test_refusals_leave_outputs_untouched(lib, entry):
    """Every GF_CHECK_ARG and the GF_ERR_UNSUPPORTED of the entry point: the documented code, the message, the sentinel-filled output as
    it was — nothing is launched.  Then the same operands are accepted.  (The operands are allocated for 64 keys and n_pad 80, so a
    refusal that failed to refuse would still stay inside its buffers.)"""
    heads, n, n_pad, sq = 2, 20, 32, 40
    D = heads * HD
    g = torch.Generator().manual_seed(3)
    rows64 = torch.randn((64, D), generator=g).to(BF).cuda()
    big = _sentinel(sq + 200, heads * 80)
    if entry == "gf_cross_probs":
        q = torch.randn((sq, D), generator=g).to(BF).cuda()
        a = dict(q=q, k=rows64, p=big, q_len=sq, n_keys=n, n_pad=n_pad, heads=heads, head_dim=HD, q_stride=D, k_stride=D, p_stride=heads * n_pad,
                 scale=float(HD ** -0.5), mult=2.0, stream=_stream())
    else:
        w = torch.randn((sq, D), generator=g).to(BF).cuda()
        a = dict(v=rows64, w=w, u=big, n_keys=n, n_pad=n_pad, heads=heads, head_dim=HD, n_out=sq, v_stride=D, w_stride=D, u_stride=heads * n_pad,
                 stream=_stream())
    table = _refusals(entry, heads, n, n_pad)
    assert len(table) >= 20
    for which, (over, code, msg) in table.items():
        if isinstance(over, str):
            name, off = over.split("+")
            over = {name: a[name].data_ptr() + int(off)}
        rc = _raw(lib, entry, a, over)
        text = lib.gf_last_error().decode()
        assert rc == code and msg in text, (entry, which, rc, text)
        assert bool((big.view(torch.int16) == SENT).all()), f"{entry} refused ({which}) and still wrote to its output"
    assert _raw(lib, entry, a) == 0, lib.gf_last_error().decode()
    assert not bool((big.view(-1)[:sq * heads * n_pad].view(torch.int16) == SENT).any())
    assert bool((big.view(-1)[sq * heads * n_pad:].view(torch.int16) == SENT).all())


def test_python_level_refusals(ops):
    """ops.cross_probs / ops.cross_fold_table refuse what the ABI cannot see (device, dtype, rank, shapes) and pass the ABI's own refusals
    on as GoalForceError with its message."""
    from goal_force_amd._lib import GoalForceError
    g = torch.Generator().manual_seed(4)
    q, k = (torch.randn((s, 256), generator=g).to(BF).cuda() for s in (40, 20))
    w = torch.randn((64, 256), generator=g).to(BF).cuda()
    bad = [
        ("must be on the GPU", lambda: ops.cross_probs(q.cpu(), k, 2, 32)), ("expected dtype", lambda: ops.cross_probs(q.float(), k, 2, 32)),
        ("expected 2-D", lambda: ops.cross_probs(q[None], k, 2, 32)), ("expected 2-D", lambda: ops.cross_probs(q[:, ::2], k[:, ::2], 1, 32)),
        ("q/k shape mismatch", lambda: ops.cross_probs(q, k[:, :128], 2, 32)), ("q/k shape mismatch", lambda: ops.cross_probs(q, k, 3, 32)),
        ("cross_probs.out: expected [40, 64]", lambda: ops.cross_probs(q, k, 2, 32, out=torch.empty((40, 96), dtype=BF, device="cuda"))),
        ("n_pad a multiple of 16", lambda: ops.cross_probs(q, k, 2, 24)), ("1 <= n_keys=20 < n_pad=16", lambda: ops.cross_probs(q, k, 2, 16)),
        ("multiplicity >= 1", lambda: ops.cross_probs(q, k, 2, 32, last_key_mult=0)), ("head_dim=64 unsupported", lambda: ops.cross_probs(q, k, 4, 32)),
        ("must be on the GPU", lambda: ops.cross_fold_table(k.cpu(), w, 2, 32)), ("expected dtype", lambda: ops.cross_fold_table(k, w.float(), 2, 32)),
        ("expected [N, 256]", lambda: ops.cross_fold_table(k, w[:, :128], 2, 32)), ("do not divide into 3 heads", lambda: ops.cross_fold_table(k, w, 3, 32)),
        ("1 <= n_keys=20 < n_pad=16", lambda: ops.cross_fold_table(k, w, 2, 16)), ("head_dim=64 unsupported", lambda: ops.cross_fold_table(k, w, 4, 32)),
    ]
    for msg, call in bad:
        with pytest.raises(GoalForceError) as e:
            call()
        assert msg in str(e.value), (msg, str(e.value))
    torch.cuda.synchronize()
    out = torch.empty((40, 64), dtype=BF, device="cuda")
    assert ops.cross_probs(q, k, 2, 32, last_key_mult=3, out=out) is out and ops.cross_fold_table(k, w, 2, 32).shape == (64, 64)


# ---------------------------------------------------------------------------------------------------------------------
# the memo
def test_context_cache_memoises_the_table(ops):
    """One tiny model_fn forward (dim 512, 4 heads: heads x n_pad = 64, a GEMM-able K) run with a ContextCache twice: the second call
    makes no cross_fold_table call, both outputs are bit-identical to a call without the cache, and every cached table equals a fresh
    fold_table bit for bit."""
    import gen_inputs as gi
    from goal_force_amd import model_fn as mf
    from goal_force_amd.dit import WanModel
    cfg = dict(gi.TINY, dim=512, num_heads=4, ffn_dim=512)
    dit = WanModel(has_image_input=False, require_clip_embedding=False, **cfg)
    dit.load_state_dict(gi.dit_sd(cfg, seed=41), strict=True)
    dit = dit.to(BF).cuda()
    inp = gi.tiny_inputs()
    ctx = torch.randn((1, 24, cfg["text_dim"]), generator=torch.Generator().manual_seed(9)).to(BF)
    ctx[:, 9:] = ctx[:, 9:10]                                   # the prompter's padding: rows 9 .. 23 identical -> 10 keys, the last x 15
    kw = dict(latents=inp["latents"].cuda(), timestep=torch.tensor([995.9], dtype=BF).cuda(), context=ctx.cuda(), y=inp["y"].cuda())
    calls = []
    real = ops.cross_fold_table
    ops.cross_fold_table = lambda *a, **k_: calls.append(1) or real(*a, **k_)
    try:
        plain = mf.model_fn_wan_video(dit, **kw)
        assert len(calls) == cfg["num_layers"], "the folded path serves every block of this model"
        cache = mf.ContextCache()
        first = mf.model_fn_wan_video(dit, context_cache=cache, **kw)
        assert len(calls) == 2 * cfg["num_layers"] and sorted(cache.dit_u) == list(range(cfg["num_layers"]))
        second = mf.model_fn_wan_video(dit, context_cache=cache, **kw)
        assert len(calls) == 2 * cfg["num_layers"], "the second call with the cache built a table again"
    finally:
        ops.cross_fold_table = real
    assert torch.equal(first, plain) and torch.equal(second, plain)
    for i, block in enumerate(dit.blocks):
        kv = cache.dit_kv[i]
        assert kv[2] == 15 and kv[0].shape[0] == 10 and block.cross_attn.fold_ok(kv)
        assert cache.dit_u[i].shape == (512, 64) and torch.equal(cache.dit_u[i], block.cross_attn.fold_table(kv))
