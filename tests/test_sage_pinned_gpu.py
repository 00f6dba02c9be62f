"""The SageAttention kernels (goal_force_amd/csrc/gf_sage_attention.hip) pinned element by element through the raw C ABI, with the
operands, the recipe and the bars of tests/sage_refs.py.

gf_sage_attn_fwd runs on hand-built codes and scales: three exact classes (`one_hot`, `uniform`, `staircase`: torch.equal with the fp32
restatement of the tail) and the Gaussian operands of the quantisers through bars (a) and (b).  Every call's operands sit in buffers
whose tails hold NaN / 0x7F, every output in a sentinel-filled buffer.  The quantisation passes are held to sage_oracle bit for bit on
hand-made blocks, gf_sage_k_mean to fp32(fp64 sum / n), gf_sage_attn to its five staged calls.  tests/test_sage_refs_cpu.py shows on
the CPU that a right restatement passes all of it and which injected faults do not.  Each comparison prints what it measured
(`pytest -s`).

Everything under test is called through `_raw`.  Two places take the thin wrappers of goal_force_amd.ops instead (they allocate the
outputs and pass the same arguments on): the operands of the gauss class and of test_tiny_blocks, and the staged half of
test_attn_is_its_five_staged_calls, whose other half is the raw gf_sage_attn."""
import math

import pytest
import torch

import attention_fwd_refs as A
import gemm_refs as G
import sage_oracle as so
import sage_refs as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HD = 128
SENT = 0x5A5A
BAD = -1                                                   # GF_ERR_INVALID_ARG
SIG = {
    "gf_sage_k_mean": "k ldk mu scratch kv_len heads stream",
    "gf_sage_quant_q": "q ldq q8 q_scale q_len heads stream",
    "gf_sage_quant_k": "k ldk mu k8 k_scale kv_len heads stream",
    "gf_sage_quant_vt": "v ldv vt_in vt8 v_scale scratch kv_len heads stream",
    "gf_sage_attn_fwd": "q8 q_scale k8 k_scale vt8 v_scale o ldo q_len kv_len heads scale stream",
    "gf_sage_attn": "q ldq k ldk v ldv vt_in o ldo q_len kv_len heads scale ws stream",
}
POINTERS = ("q", "k", "v", "o", "mu", "scratch", "q8", "q_scale", "k8", "k_scale", "vt8", "v_scale", "ws")


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


def _guarded(t, extra=4096):
    """t on the GPU as the head of a buffer whose tail holds NaN (floats) or 0x7F (codes: 127, and the e4m3 NaN code)."""
    flat = torch.empty((t.numel() + extra,), dtype=t.dtype, device="cuda")
    flat.fill_(math.nan if t.dtype.is_floating_point else 0x7F)
    flat[:t.numel()].copy_(t.reshape(-1))
    return flat[:t.numel()].view(t.shape)


def _out_guard(shape, dtype, extra=1024):
    """A sentinel-filled output buffer (bytes 0x5A) with `extra` elements behind -> (view, flat)."""
    n = math.prod(shape)
    flat = torch.empty((n + extra,), dtype=dtype, device="cuda")
    flat.view(torch.uint8).fill_(0x5A)
    return flat[:n].view(shape), flat


def _tail_intact(flat, n):
    return bool((flat[n:].view(torch.uint8) == 0x5A).all())


def _fwd_args(op, dev, o, **more):
    a = dict(q8=dev["q8"], q_scale=dev["qs"], k8=dev["k8"], k_scale=dev["ks"], vt8=dev["vt8"], v_scale=dev["vs"], o=o, ldo=o.stride(0),
             q_len=op.q_len, kv_len=op.kv_len, heads=op.heads, scale=float(op.scale), stream=_stream())
    a.update(more)
    return a


def _upload(op):
    return {n: _guarded(getattr(op, n)) for n in ("q8", "qs", "k8", "ks", "vt8", "vs")}


def _fwd(lib, op, gap=0):
    """gf_sage_attn_fwd on guarded operands -> O [q_len, H*128] bf16 on the CPU; ldo = H*128 + gap, the gap and two rows behind intact."""
    D = op.heads * HD
    obuf = _sentinel(op.q_len + 2, D + gap)
    assert _raw(lib, "gf_sage_attn_fwd", _fwd_args(op, _upload(op), obuf[:op.q_len, :D])) == 0, lib.gf_last_error().decode()
    oi = obuf.view(torch.int16)
    assert bool((oi[op.q_len:] == SENT).all()), "rows >= q_len were written"
    assert bool((oi[:, D:] == SENT).all()), "the gap between two rows of O was written"
    assert not bool((oi[:op.q_len, :D] == SENT).any()), "an element of O was not written"
    return obuf[:op.q_len, :D].cpu()


def _eq(a, b):
    return torch.equal(a.float(), b.float())                # -0 == +0: a sum of exact zeros has no stated sign


# ---------------------------------------------------------------------------------------------------------------------
# gf_sage_attn_fwd: the exact classes
@pytest.mark.parametrize("where", ["first", "last", "spread"])
def test_one_hot(lib, where):
    """O[row] is the hot key's V code times v_scale bit for bit: the V^T permutation, the D-fragment map, the LDS-swizzled epilogue, the
    ring and, with the hot key behind the first tile, an alpha that underflows to exactly 0.  Rests on exp2(8) = 256 exactly.  The cases
    hold every kv_len edge (whole and ragged last tiles and 64-key halves, the lane group, the 16-key block) and every q_len edge."""
    for q_len, kv, heads, shift in R.ONE_HOT_CASES:
        op, hot, want = R.one_hot(q_len, kv, heads, where, shift)
        msg = R.one_hot_report(_fwd(lib, op), op, hot, want, shift)
        assert msg is None, f"[{where}] {msg}"


@pytest.mark.parametrize("variant", ["q0", "qs0", "ks0"])
def test_uniform_every_key_count(lib, variant):
    """Every P is 256, acc = 256 sum V and l = 256 n exactly: one key too many or too few changes every element.  kv_len 1 .. 130 and
    the later tile edges; on every third length the padding holds garbage and the scale of an all-pad half is NaN."""
    for kv in R.UNIFORM_KV:
        op, want = R.uniform(33, kv, 2, variant, garbage=(kv % 3 == 0))
        got = _fwd(lib, op)
        assert _eq(got, want), f"uniform {variant} keys={kv}: {int((got.float() != want.float()).sum())} of {want.numel()} elements differ from tail(256 sum V, 256 n)"
    for q_len in R.Q_LENS:
        for kv, heads in ((97, 3), (129, 5)):
            op, want = R.uniform(q_len, kv, heads, variant, garbage=True)
            assert _eq(_fwd(lib, op, gap=8), want), f"uniform {variant} q={q_len} keys={kv} heads={heads}"


@pytest.mark.parametrize("nt", [2, 3, 4, 5])
def test_staircase(lib, nt):
    """Integer scores whose tile maxima rise by 1 .. 5 and fall: every alpha a power of two, every fp32 step exact up to the tail."""
    for q_len, kv, heads in ((129, 128 * nt, 3), (257, 128 * nt - 61, 3), (33, 128 * nt - 127, 1)):
        op = R.staircase(q_len, nt, heads, kv)
        want, got = R.restate(op), _fwd(lib, op)
        bad = torch.nonzero(got.float() != want.float())
        assert not len(bad), (f"staircase tiles={nt} q={q_len} keys={kv}: {len(bad)} elements differ, first (row, column) {bad[0].tolist()}: "
                              f"{float(got[tuple(bad[0])])} for {float(want[tuple(bad[0])])}")


# ---------------------------------------------------------------------------------------------------------------------
# gf_sage_attn_fwd: the gauss class
def _gauss_ops(ops, sq, skv, heads, std, blocks, seed=0):
    """The operands ops.sage_quant_q / _k / _vt produce from gauss_qkv, as a CPU Ops."""
    q, k, v = (t.cuda() for t in R.gauss_qkv(sq, skv, heads, std, seed, blocks))
    q8, qs = ops.sage_quant_q(q, heads)
    k8, ks, _ = ops.sage_quant_k(k, heads)
    vt8, vs = ops.sage_quant_vt(v, heads)
    torch.cuda.synchronize()
    return R.Ops(q8.cpu(), qs.cpu(), k8.cpu(), ks.cpu(), vt8.cpu(), vs.cpu(), sq, skv, heads, HD ** -0.5)


@pytest.mark.parametrize("i", range(len(R.gauss_cases())))
def test_gauss_edges(ops, lib, i):
    sq, skv, heads, std, blocks = R.gauss_cases()[i]
    op = _gauss_ops(ops, sq, skv, heads, std, blocks)
    R.assert_pinned(_fwd(lib, op), R.recipe(op), f"gauss q={sq} keys={skv} heads={heads} std={std:g} blocks={blocks}")


@pytest.mark.parametrize("heads,q_len", [(8, 200), (8, 300), (16, 200), (16, 257)])
def test_xcd_ordered_grid(ops, lib, heads, q_len):
    """Each head of the XCD-ordered grid (heads 8 and 16, 2 and 3 query blocks) equals that head run alone, bit for bit."""
    op = _gauss_ops(ops, q_len, 257, heads, 1.0, False)
    full = _fwd(lib, op).view(q_len, heads, HD)
    for h in range(heads):
        c = slice(h * HD, h * HD + HD)
        one = R.Ops(op.q8[:, c].contiguous(), op.qs[h:h + 1].contiguous(), op.k8[:, c].contiguous(), op.ks[h:h + 1].contiguous(),
                    op.vt8[c].contiguous(), op.vs[h:h + 1].contiguous(), q_len, 257, 1, op.scale)
        assert torch.equal(_fwd(lib, one).view(torch.int16), full[:, h].contiguous().view(torch.int16)), f"head {h} of {heads}, q={q_len}"


# ---------------------------------------------------------------------------------------------------------------------
# memory discipline of gf_sage_attn_fwd
@pytest.mark.parametrize("sq,skv,heads", [(129, 97, 3), (33, 130, 1), (257, 385, 5)])
def test_memory_discipline(ops, lib, sq, skv, heads):
    """ldo = heads*128 + 8 and + 16 with the gap and the rows behind intact; garbage in the pad rows of k8 and (finite: the header asks
    for zeros there, and 0 x an e4m3 NaN code would be NaN) in the pad positions of vt8, a NaN k_scale on an all-pad half: the same bits;
    q_len = 0 returns OK and writes nothing."""
    op = _gauss_ops(ops, sq, skv, heads, 1.0, False)
    want = _fwd(lib, op)
    for gap in (8, 16):
        assert torch.equal(_fwd(lib, op, gap).view(torch.int16), want.view(torch.int16)), f"O changed with ldo = heads*128 + {gap}"
    g = torch.Generator().manual_seed(skv)
    dirty = op._replace(k8=op.k8.clone(), vt8=op.vt8.clone(), ks=op.ks.clone())
    dirty.k8[skv:] = torch.randint(-127, 128, (dirty.k8.shape[0] - skv, heads * HD), generator=g).to(torch.int8)
    pad = torch.ones(dirty.vt8.shape[1], dtype=torch.bool)
    pad[so.vt_position(skv)] = False
    dirty.vt8[:, pad] = R.FINITE[torch.randint(0, len(R.FINITE), (heads * HD, int(pad.sum())), generator=g)]
    if skv % 128 and skv % 128 <= 64:
        dirty.ks[:, -1] = math.nan
    assert torch.equal(_fwd(lib, dirty).view(torch.int16), want.view(torch.int16)), "O depends on what the padding of k8 / vt8 / k_scale holds"
    obuf = _sentinel(sq, heads * HD)
    assert _raw(lib, "gf_sage_attn_fwd", _fwd_args(op, _upload(op), obuf), dict(q_len=0)) == 0, lib.gf_last_error().decode()
    assert bool((obuf.view(torch.int16) == SENT).all()), "q_len == 0 wrote something"


# ---------------------------------------------------------------------------------------------------------------------
# the quantisation passes
def _scratch(heads):
    return torch.empty((heads * 64 * 128 * 8,), dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("rows", R.MEAN_ROWS)
def test_k_mean_exact(lib, rows):
    """fp32(fp64 sum / n) bit for bit on data whose fp64 sum is exact, k a strided slice of a NaN parent; rows = 65 has empty chunks."""
    heads = 2
    k = R.exact_mean_k(rows, heads)
    kd = A.embed(k.cuda(), 3, 8, 16)
    mu, flat = _out_guard((heads, HD), torch.float32)
    a = dict(k=kd, ldk=kd.stride(0), mu=mu, scratch=_scratch(heads), kv_len=rows, heads=heads, stream=_stream())
    assert _raw(lib, "gf_sage_k_mean", a) == 0, lib.gf_last_error().decode()
    assert _tail_intact(flat, heads * HD)
    assert torch.equal(mu.cpu(), R.k_mean(k, heads)), f"rows={rows}: {int((mu.cpu() != R.k_mean(k, heads)).sum())} means differ"


def _hand_blocks(rows, heads, seed, blk):
    """bf16 [rows, H*128] in scale blocks of `blk` rows: block 0 holds k + 0.5 (k = -127 .. 126) and +-127 (amax 127, inv 1: ties to
    even, the clamp's edge), block 1 zeros, block 2 Gaussian x 2^60, block 3 Gaussian x 2^-60, the rest Gaussian."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, heads * HD), generator=g)
    n0 = min(blk, rows)
    x[:n0] = (torch.randint(-127, 127, (n0, heads * HD), generator=g) + 0.5)
    x[0, ::3] = 127.0
    x[0, 1::3] = -127.0
    x[blk:2 * blk] = 0.0
    x[2 * blk:3 * blk] *= 2.0 ** 60
    x[3 * blk:4 * blk] *= 2.0 ** -60
    return x.to(BF)


def _hand_checks(x, codes, scales, rows, blk):
    """The named cases, stated without the oracle: block 0 is rne(x) clamped with scale 1, a whole zero block 1 has scale 0 and codes 0,
    block 2 lies 2^60 above and block 3 2^-60 below a Gaussian block's scale."""
    if rows >= blk:
        assert torch.equal(codes[:blk].float(), torch.round(x[:blk].float()).clamp(-127, 127)) and bool((scales[:, 0] == 1.0).all()), "block 0"
        assert bool((codes[:blk].abs() == 127).any()) and bool(((x[:blk].float().abs() % 1.0) == 0.5).any())
    if rows >= 2 * blk:
        assert float(scales[:, 1].abs().max()) == 0.0 and int(codes[blk:2 * blk].abs().max()) == 0, "the all-zero block"
    if rows > 4 * blk:
        assert bool((scales[:, 2] > 2.0 ** 50 * scales[:, 4]).all()) and bool((scales[:, 3] < 2.0 ** -50 * scales[:, 4]).all())
        assert int(codes[2 * blk:4 * blk].abs().max()) == 127


@pytest.mark.parametrize("fill", [math.nan, 3e38])
@pytest.mark.parametrize("rows", [7, 32, 33, 135, 257])
def test_quant_q_hand_made_blocks(lib, rows, fill):
    """q a strided slice of a parent filled with NaN (what the issue asks) or with 3e38 (the sharper probe of the short last block:
    fmaxf drops a NaN, so an absent row that entered the amax would show only with a huge finite value)."""
    heads = 3
    q = _hand_blocks(rows, heads, rows, 32)
    want8, wants = so.quant_q(q, heads)
    qd = A.embed(q.cuda(), 3, 8, 8, fill=fill)
    q8, f8 = _out_guard((rows, heads * HD), torch.int8)
    qs, fs = _out_guard(wants.shape, torch.float32)
    a = dict(q=qd, ldq=qd.stride(0), q8=q8, q_scale=qs, q_len=rows, heads=heads, stream=_stream())
    assert _raw(lib, "gf_sage_quant_q", a) == 0, lib.gf_last_error().decode()
    assert _tail_intact(f8, q8.numel()) and _tail_intact(fs, qs.numel()), "gf_sage_quant_q wrote behind q8 or q_scale"
    assert torch.equal(qs.cpu(), wants), "q_scale"
    assert torch.equal(q8.cpu().view(rows, heads, HD).transpose(0, 1), want8), "q8"
    _hand_checks(q, q8.cpu(), qs.cpu(), rows, 32)


@pytest.mark.parametrize("fill", [math.nan, 3e38])
@pytest.mark.parametrize("rows,zero_mu", [(7, True), (64, True), (65, True), (135, True), (257, True), (300, True), (135, False), (300, False)])
def test_quant_k_hand_made_blocks(lib, rows, zero_mu, fill):
    """The same blocks laid out for K's 64-row scale blocks.  mu = 0: k~ = k, so the ties, the clamp, the all-zero middle block and the
    2^+-60 blocks are met as built (and stated without the oracle); a Gaussian mu on the odd channels: the subtraction, against the oracle."""
    heads = 3
    k = _hand_blocks(rows, heads, 1000 + rows, 64)
    mu = torch.zeros((heads, HD))
    if not zero_mu:
        mu[:, 1::2] = 0.25 * torch.randn((heads, HD // 2), generator=torch.Generator().manual_seed(rows))
    want8, wants = so.quant_k(k, heads, mu)
    kd = A.embed(k.cuda(), 3, 8, 8, fill=fill)
    kvp = R.pad128(rows)
    k8, f8 = _out_guard((kvp, heads * HD), torch.int8)
    ks, fs = _out_guard((heads, kvp // 64), torch.float32)
    a = dict(k=kd, ldk=kd.stride(0), mu=mu.cuda(), k8=k8, k_scale=ks, kv_len=rows, heads=heads, stream=_stream())
    assert _raw(lib, "gf_sage_quant_k", a) == 0, lib.gf_last_error().decode()
    assert _tail_intact(f8, k8.numel()) and _tail_intact(fs, ks.numel()), "gf_sage_quant_k wrote behind k8 or k_scale"
    nb = wants.shape[1]
    assert torch.equal(ks.cpu()[:, :nb], wants) and float(ks.cpu()[:, nb:].abs().sum()) == 0.0, "k_scale (an all-pad block has scale 0)"
    assert torch.equal(k8.cpu()[:rows].view(rows, heads, HD).transpose(0, 1), want8), "k8"
    assert int(k8.cpu()[rows:].abs().sum()) == 0, "rows in [kv_len, kv_pad8) are not code 0"
    if zero_mu:
        _hand_checks(k, k8.cpu()[:rows], ks.cpu(), rows, 64)


@pytest.mark.parametrize("amax", R.TINY)
def test_tiny_blocks(ops, lib, amax):
    """Blocks (Q, K) and channels (V) whose amax is 2^-120, 2^-126 or bf16's smallest subnormal, zeros beside the tiny values: the
    header's tiny-block rule — the oracle's codes and scales bit for bit, code 0 for every zero, no e4m3 NaN code, a finite O."""
    heads, rows = 2, 130
    x = R.tiny_rows(rows, heads, amax)
    zero = (x == 0).view(rows, heads, HD).transpose(0, 1)
    xd = x.cuda()
    q8, qs = ops.sage_quant_q(xd, heads)
    w8, ws = so.quant_q(x, heads)
    assert torch.equal(q8.cpu().view(rows, heads, HD).transpose(0, 1), w8) and torch.equal(qs.cpu(), ws), "q"
    assert int(q8.cpu().view(rows, heads, HD).transpose(0, 1)[zero].abs().sum()) == 0 and bool((qs > 0).all())
    mu = ops.sage_k_mean(xd, heads)
    assert float(mu.abs().max()) == 0.0
    k8, ks, _ = ops.sage_quant_k(xd, heads, mu)
    w8, ws = so.quant_k(x, heads, mu.cpu())
    assert torch.equal(k8.cpu()[:rows].view(rows, heads, HD).transpose(0, 1), w8) and torch.equal(ks.cpu()[:, :ws.shape[1]], ws), "k"
    assert int(k8.cpu()[:rows].view(rows, heads, HD).transpose(0, 1)[zero].abs().sum()) == 0
    vt8, vs = ops.sage_quant_vt(xd, heads)
    want8, wantvs = R.quant_vt_ref(x, heads)
    assert not bool(((vt8 & 0x7F) == 0x7F).any()), "an e4m3 NaN code in vt8"
    assert torch.equal(vt8.cpu(), want8) and torch.equal(vs.cpu(), wantvs), "vt8 / v_scale"
    q, k, _ = (t.cuda() for t in R.gauss_qkv(33, rows, heads, 1.0))
    o = ops.sage_attn(q, k, xd, heads)
    assert bool(torch.isfinite(o.float()).all()), "gf_sage_attn on a V of tiny channels is not finite"
    assert float(o.float().abs().max()) <= amax, "O is a convex combination of V"


@pytest.mark.parametrize("kv", R.VT_KV)
def test_quant_vt_both_inputs(lib, kv):
    """Plain V (a strided slice of a NaN parent) and the bf16 V^T in the vt32 layout built on the host (positions past kv_len NaN, ldv
    with a gap of 64): codes at vt_position equal to quant_v, pad positions 0, scales equal."""
    heads = 2
    v = R.gauss_qkv(1, kv, heads, 1.0, seed=kv)[2]
    v[:, 5] = 0.0
    want8, wants = R.quant_vt_ref(v, heads)
    kvp = R.pad128(kv)
    vt32 = R.vt32_of(v)
    vt32[:, G.vt_positions(vt32.shape[1])[kv:]] = math.nan
    wide = torch.full((heads * HD, vt32.shape[1] + 64), math.nan, dtype=BF)
    wide[:, :vt32.shape[1]] = vt32
    for what, src, ldv, vt_in in (("V", A.embed(v.cuda(), 3, 8, 16), None, 0), ("V^T", vt32.cuda(), vt32.shape[1], 1), ("V^T, ldv + 64", wide.cuda(), wide.shape[1], 1)):
        vt8, f8 = _out_guard((heads * HD, kvp), torch.uint8)
        vs, fs = _out_guard((heads, HD), torch.float32)
        a = dict(v=src, ldv=src.stride(0) if ldv is None else ldv, vt_in=vt_in, vt8=vt8, v_scale=vs, scratch=_scratch(heads), kv_len=kv, heads=heads,
                 stream=_stream())
        assert _raw(lib, "gf_sage_quant_vt", a) == 0, lib.gf_last_error().decode()
        assert _tail_intact(f8, vt8.numel()) and _tail_intact(fs, vs.numel()), f"{what}: wrote behind vt8 or v_scale"
        assert torch.equal(vs.cpu(), wants), f"{what} keys={kv}: v_scale"
        assert torch.equal(vt8.cpu(), want8), f"{what} keys={kv}: {int((vt8.cpu() != want8).sum())} codes differ (pad positions are 0 in the expectation)"


# ---------------------------------------------------------------------------------------------------------------------
# the composition
def _attn_args(q, k, v, ldv, vt_in, o, ws, sq, skv, heads, scale):
    return dict(q=q, ldq=q.stride(0), k=k, ldk=k.stride(0), v=v, ldv=ldv, vt_in=vt_in, o=o, ldo=o.stride(0), q_len=sq, kv_len=skv, heads=heads,
                scale=scale, ws=ws, stream=_stream())


@pytest.mark.parametrize("sq,skv,heads", [(129, 97, 3), (33, 257, 2)])
def test_attn_is_its_five_staged_calls(ops, lib, sq, skv, heads):
    """gf_sage_attn (vt_in 0 and 1) equals k_mean, quant_q, quant_k, quant_vt, attn_fwd called one by one, bit for bit, inside a
    workspace of exactly gf_sage_workspace_bytes with a sentinel page behind it."""
    q, k, v = (t.cuda() for t in R.gauss_qkv(sq, skv, heads, 1.0, 3, False))
    vt32 = R.vt32_of(v.cpu()).cuda()
    scale = float(HD ** -0.5)
    mu = ops.sage_k_mean(k, heads)
    q8, qs = ops.sage_quant_q(q, heads)
    k8, ks, _ = ops.sage_quant_k(k, heads, mu)
    vt8, vs = ops.sage_quant_vt(v, heads)
    staged = ops.sage_attn_quantized(q8, qs, k8, ks, vt8, vs, skv, heads)
    nbytes = int(lib.gf_sage_workspace_bytes(sq, skv, heads))
    kvp, nqs = R.pad128(skv), -(-sq // 32)
    p256 = lambda n: -(-n // 256) * 256                                                             # noqa: E731
    assert nbytes == sum(p256(n) for n in (sq * heads * HD, kvp * heads * HD, heads * HD * kvp, heads * nqs * 4, heads * (kvp // 64) * 4,
                                           heads * HD * 4, heads * HD * 4, heads * 64 * HD * 8)), "the header's workspace layout"
    for vt_in, src, ldv in ((0, v, v.stride(0)), (1, vt32, vt32.shape[1])):
        ws, flat = _out_guard((nbytes,), torch.uint8, extra=4096)
        o = _sentinel(sq, heads * HD)
        assert _raw(lib, "gf_sage_attn", _attn_args(q, k, src, ldv, vt_in, o, ws, sq, skv, heads, scale)) == 0, lib.gf_last_error().decode()
        assert _tail_intact(flat, nbytes), "gf_sage_attn wrote behind its workspace"
        assert torch.equal(o.view(torch.int16), staged.view(torch.int16)), f"vt_in={vt_in}: gf_sage_attn is not its five staged calls"


def test_attn_constant_k_is_uniform(ops):
    """k constant along the keys: k~ = 0 exactly, every P is 256, O = tail(256 sum V_code, 256 n) of the V codes quant_vt wrote."""
    sq, skv, heads = 33, 97, 2
    g = torch.Generator().manual_seed(4)
    q = R.gauss_qkv(sq, skv, heads, 1.0, 4, False)[0].cuda()
    k = R.gauss_qkv(1, 1, heads, 1.0, 5, False)[1].cuda().expand(skv, heads * HD).contiguous()
    v = torch.randint(1, 8, (skv, heads * HD), generator=g) * (2 * torch.randint(0, 2, (skv, heads * HD), generator=g) - 1)
    v[0] = 7                                                # amax 7: the reciprocal is 64, every code 64 v is an e4m3 value, the sums exact
    v = v.to(BF).cuda()
    vt8, vs = ops.sage_quant_vt(v, heads)
    assert torch.equal(R.decode(vt8.cpu())[:, so.vt_position(skv)].t(), 64.0 * v.cpu().double()) and bool((vs == 2.0 ** -6).all())
    codes = R.decode(vt8.cpu()).view(heads, HD, -1).sum(-1)                                          # pad positions are 0
    assert bool(((256.0 * codes).float().double() == 256.0 * codes).all())
    want = torch.stack([R.tail((256.0 * codes[h]).float()[None], torch.tensor([256.0 * skv]), vs.cpu()[h]) for h in range(heads)], 1)
    got = ops.sage_attn(q, k, v, heads).cpu()
    assert _eq(got, want.expand(sq, heads, HD).reshape(sq, -1)), "a constant k does not give the uniform expectation"


# ---------------------------------------------------------------------------------------------------------------------
# refusals
def test_refusals_leave_outputs_untouched(ops, lib):
    """Every refusal of the seven entry points (88: 61 of the passes and gf_sage_attn, 23 of gf_sage_attn_fwd, 4 of
    gf_sage_workspace_bytes) by code and message, every output buffer as it was.  The operands are allocated for the
    accepted call, and every refusal returns before a launch — but for gf_sage_attn's inner ones (ldq / ldo), which may follow the
    earlier stages' writes into the workspace and must leave o alone (include/goalforce.h)."""
    heads, sq, skv = 2, 40, 70
    D, kvp = heads * HD, 128
    q, k, v = (t.cuda() for t in R.gauss_qkv(sq, skv, heads, 1.0, 6, False))
    vt32 = R.vt32_of(v.cpu()).cuda()
    outs = dict(mu=torch.float32, q8=torch.int8, q_scale=torch.float32, k8=torch.int8, k_scale=torch.float32, vt8=torch.uint8, v_scale=torch.float32,
                o=BF, ws=torch.uint8)
    n = dict(mu=heads * HD, q8=sq * D, q_scale=heads * 2, k8=kvp * D, k_scale=heads * 2, vt8=D * kvp, v_scale=heads * HD, o=sq * D,
             ws=int(lib.gf_sage_workspace_bytes(sq, skv, heads)))
    buf = {name: _out_guard((n[name],), dt, extra=256) for name, dt in outs.items()}
    b = {name: view for name, (view, _) in buf.items()}
    scratch, muv = _scratch(heads), torch.zeros((heads, HD), device="cuda")
    st, nan, inf = _stream(), float("nan"), float("inf")
    E = {
        "gf_sage_k_mean": dict(k=k, ldk=D, mu=b["mu"], scratch=scratch, kv_len=skv, heads=heads, stream=st),
        "gf_sage_quant_q": dict(q=q, ldq=D, q8=b["q8"], q_scale=b["q_scale"], q_len=sq, heads=heads, stream=st),
        "gf_sage_quant_k": dict(k=k, ldk=D, mu=muv, k8=b["k8"], k_scale=b["k_scale"], kv_len=skv, heads=heads, stream=st),
        "gf_sage_quant_vt": dict(v=v, ldv=D, vt_in=0, vt8=b["vt8"], v_scale=b["v_scale"], scratch=scratch, kv_len=skv, heads=heads, stream=st),
        "gf_sage_attn": dict(q=q, ldq=D, k=k, ldk=D, v=v, ldv=D, vt_in=0, o=b["o"].view(sq, D), ldo=D, q_len=sq, kv_len=skv, heads=heads,
                             scale=0.1, ws=b["ws"], stream=st),
    }
    shape = lambda e: f"{e}: bad shape"                                                              # noqa: E731
    table = []
    for e, x, ld, length in (("gf_sage_k_mean", "k", "ldk", "kv_len"), ("gf_sage_quant_q", "q", "ldq", "q_len"), ("gf_sage_quant_k", "k", "ldk", "kv_len")):
        table += [(e, {x: None}, f"{e}: null pointer"), (e, {"heads": 0}, shape(e)), (e, {length: 0}, shape(e)), (e, {length: -1}, shape(e)),
                  (e, {ld: D - 8}, shape(e)), (e, {ld: D + 4}, shape(e)), (e, {x: E[e][x].data_ptr() + 8}, shape(e)), (e, {length: 1 << 24}, shape(e))]
    table += [("gf_sage_k_mean", {"mu": None}, "gf_sage_k_mean: null pointer"), ("gf_sage_k_mean", {"scratch": None}, "gf_sage_k_mean: null pointer"),
              ("gf_sage_quant_q", {"q8": None}, "gf_sage_quant_q: null pointer"), ("gf_sage_quant_q", {"q_scale": None}, "gf_sage_quant_q: null pointer"),
              ("gf_sage_quant_q", {"q8": b["q8"].data_ptr() + 8}, shape("gf_sage_quant_q")),
              ("gf_sage_quant_k", {"mu": None}, "gf_sage_quant_k: null mu"), ("gf_sage_quant_k", {"k8": None}, "gf_sage_quant_k: null pointer"),
              ("gf_sage_quant_k", {"k_scale": None}, "gf_sage_quant_k: null pointer"), ("gf_sage_quant_k", {"k8": b["k8"].data_ptr() + 8}, shape("gf_sage_quant_k"))]
    e = "gf_sage_quant_vt"
    kvneed = f"{e}: V^T input needs kv_pad"
    table += [(e, {"v": None}, f"{e}: null pointer"), (e, {"vt8": None}, f"{e}: null pointer"), (e, {"v_scale": None}, f"{e}: null pointer"),
              (e, {"scratch": None}, f"{e}: null pointer"), (e, {"heads": 0}, shape(e)), (e, {"kv_len": 0}, shape(e)), (e, {"kv_len": 1 << 24}, shape(e)),
              (e, {"ldv": D + 4}, shape(e)), (e, {"ldv": D - 8}, f"{e}: ldv="), (e, {"v": v.data_ptr() + 8}, shape(e)), (e, {"vt8": b["vt8"].data_ptr() + 8}, shape(e)),
              (e, {"v": vt32, "vt_in": 1, "ldv": 64}, kvneed), (e, {"v": vt32, "vt_in": 1, "ldv": 96}, kvneed), (e, {"v": vt32, "vt_in": 1, "ldv": 72}, kvneed)]
    e = "gf_sage_attn"
    bad_scale = f"{e}: the softmax scale must be positive and finite"
    table += [(e, {"ws": None}, f"{e}: null workspace"), (e, {"scale": 0.0}, bad_scale), (e, {"scale": -1.0}, bad_scale), (e, {"scale": inf}, bad_scale),
              (e, {"scale": nan}, bad_scale), (e, {"heads": 0}, f"{e}: bad lengths"), (e, {"kv_len": 0}, f"{e}: bad lengths"), (e, {"q_len": -1}, f"{e}: bad lengths"),
              (e, {"kv_len": 1 << 24}, f"{e}: bad lengths"), (e, {"k": None}, "gf_sage_k_mean: null pointer"), (e, {"ldk": D - 8}, shape("gf_sage_k_mean")),
              (e, {"ldq": D - 8}, shape("gf_sage_quant_q")), (e, {"ldo": D - 8}, shape("gf_sage_attn_fwd")), (e, {"ldo": D + 4}, shape("gf_sage_attn_fwd"))]
    assert len(table) == 61

    def untouched(skip=()):
        return all(bool((flat.view(torch.uint8) == 0x5A).all()) for name, (_, flat) in buf.items() if name not in skip)

    for entry, over, msg in table:
        rc = _raw(lib, entry, E[entry], over)
        text = lib.gf_last_error().decode()
        assert rc == BAD and msg in text, (entry, over, rc, text)
        inner = entry == "gf_sage_attn" and not msg.startswith("gf_sage_attn:") and not msg.startswith("gf_sage_k_mean")
        assert untouched(skip=("ws",) if inner else ()), f"{entry} refused ({over}) and still wrote to an output"
        if inner:
            buf["ws"][1].view(torch.uint8).fill_(0x5A)
    # gf_sage_attn_fwd, on operands of its own
    op = _gauss_ops(ops, sq, skv, heads, 1.0, False)
    dev = _upload(op)
    a = _fwd_args(op, dev, b["o"].view(sq, D))
    e = "gf_sage_attn_fwd"
    bad_scale = f"{e}: the softmax scale must be positive and finite"
    fwd = [({p: None}, f"{e}: null pointer") for p in ("q8", "q_scale", "k8", "k_scale", "vt8", "v_scale", "o")]
    fwd += [({"heads": 0}, shape(e)), ({"kv_len": 0}, shape(e)), ({"q_len": -1}, shape(e)), ({"kv_len": 1 << 24}, shape(e)), ({"q_len": 1 << 24}, shape(e)),
            ({"ldo": D - 8}, shape(e)), ({"ldo": D + 4}, shape(e)), ({"scale": 0.0}, bad_scale), ({"scale": -0.5}, bad_scale), ({"scale": inf}, bad_scale),
            ({"scale": nan}, bad_scale)]
    fwd += [({p: a[p].data_ptr() + 8}, shape(e)) for p in ("q8", "k8", "vt8", "o", "v_scale")]
    assert len(fwd) == 23                                   # with the four gf_sage_workspace_bytes checks below: 88 refusals
    for over, msg in fwd:
        rc = _raw(lib, e, a, over)
        text = lib.gf_last_error().decode()
        assert rc == BAD and msg in text, (e, over, rc, text)
        assert untouched(), f"{e} refused ({over}) and still wrote to O"
    for bad in ((-1, skv, heads), (sq, 0, heads), (sq, -3, heads), (sq, skv, 0)):
        assert int(lib.gf_sage_workspace_bytes(*bad)) == 0, bad
    # the same operands are accepted
    for entry in ("gf_sage_k_mean", "gf_sage_quant_q", "gf_sage_quant_k", "gf_sage_quant_vt", "gf_sage_attn"):
        assert _raw(lib, entry, E[entry]) == 0, lib.gf_last_error().decode()
    assert _raw(lib, e, a) == 0, lib.gf_last_error().decode()
    for name, (_, flat) in buf.items():
        assert _tail_intact(flat, n[name]), f"the accepted calls wrote behind {name}"
