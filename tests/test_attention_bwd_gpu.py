"""The attention backward (goal_force_amd/csrc/gf_attention_bwd.hip: the delta, dQ and dK/dV kernels) pinned element by element against the
fp64 reference of tests/attention_bwd_refs.py at every tile, ring and grid edge, on the data classes where it can go wrong, and with its
memory discipline and refusals checked through the raw C ABI.

The kernels are fed the exact o and lse rounded once (R.kernel_inputs), so only the backward is on the bill.  Every gradient is held to
    |got - ref| <= u |ref| + u W + 2^-16 rms(ref row)        (u = 2^-8; W: the worst case of the operand roundings and of delta's)
and every (row, head) to the row bar: error norm <= 1.25 x the worst ratio an fp32 restatement of the chain reaches over these very cases
against the predicted rounding noise (both derived in the helper; tests/test_attention_bwd_refs_cpu.py shows on the CPU that the right
chain passes all of it and that a key row 5 % off, a dropped last key, a shifted granule record, a transposed lse and a second rounding
do not).  Each test prints its worst element and row ratio (`pytest -s`).

Edges (head_dim 128): dQ — 16-query block, 32-query wave, 256-query workgroup, 32-key half-tile descriptors, 64-key tiles in a loop
unrolled by two; dK/dV — 16-key block, 48-key wave pair, 192-key workgroup, 32-query granules in a ring of 4 requested two ahead (wrap at
4 and 8 granules, wave B's drain, the clamped record index at odd granule counts); the XCD-ordered (head, block) decode at heads % 8 == 0.
"""
import pytest
import torch

import attention_bwd_refs as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HD = R.HD
SENT = 0x5A5A                # a finite bf16 bit pattern (1.5e16) no gradient here comes near
GF_ERR_INVALID_ARG, GF_ERR_UNSUPPORTED = -1, -2


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


def _case(name, sq, skv, heads):
    """((q, k, v, dout) on the CPU, scale, reference): computed once per case and left unchanged."""
    key = (name, sq, skv, heads)
    if key not in _CACHE:
        q, k, v, dout, scale = R.case_inputs(name, sq, skv, heads, torch.Generator().manual_seed(R.case_seed(*key)))
        _CACHE[key] = ((q, k, v, dout), scale, R.grads_ref(q, k, v, dout, heads, scale))
    return _CACHE[key]


def _dev(case):
    """(q, k, v, o, dout, lse) on the GPU, o and lse from the exact reference."""
    (q, k, v, dout), _, ref = case
    o, lse = R.kernel_inputs(ref)
    return tuple(t.cuda() for t in (q, k, v, o, dout, lse))


def _run(ops, case, **kw):
    q, k, v, o, dout, lse = _dev(case)
    got = ops.flash_attn_bwd(q, k, v, o, dout, lse, case[2].heads, scale=case[1], **kw)
    torch.cuda.synchronize()
    return got


def _cpu(got3):
    return tuple(t.cpu() for t in got3)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# tile and ring edges
@pytest.mark.parametrize("sq,skv", R.TILE_PAIRS)
def test_tile_and_ring_edges(ops, sq, skv):
    for heads in R.TILE_HEADS:
        case = _case("std1", sq, skv, heads)
        got = _cpu(_run(ops, case))
        for t, n in zip(got, (sq, skv, skv)):
            assert t.dtype == BF and tuple(t.shape) == (n, heads * HD)
        R.assert_within(got, case[2], f"EDGE q={sq} kv={skv} heads={heads}")
        if skv == 1:           # one key: P = 1, dS = 0 in exact math — the bound's absolute terms are all that is allowed
            assert float(case[2].dq.abs().max()) < 1e-12 and float(case[2].dk.abs().max()) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# the XCD-ordered grid
@pytest.mark.parametrize("sq,skv,heads", R.XCD_CASES)
def test_xcd_ordered_grid(ops, sq, skv, heads):
    """heads % 8 == 0 with at least two query or key blocks per head: per element against fp64, and bit-identical, head by head, to that
    head run alone (heads = 1 on a strided column slice) — which pins the (head, block) decode exactly."""
    case = _case("std1", sq, skv, heads)
    q, k, v, o, dout, lse = _dev(case)
    got = ops.flash_attn_bwd(q, k, v, o, dout, lse, heads, scale=case[1])
    R.assert_within(_cpu(got), case[2], f"XCD q={sq} kv={skv} heads={heads}")
    for h in range(heads):
        c = slice(h * HD, (h + 1) * HD)
        one = ops.flash_attn_bwd(q[:, c], k[:, c], v[:, c], o[:, c], dout[:, c], lse[:, h:h + 1].contiguous(), 1, scale=case[1])
        for name, a, b in zip(("dq", "dk", "dv"), got, one):
            assert _same(a[:, c], b), f"head {h} of {heads}: {name} differs from the head run alone"


# ---------------------------------------------------------------------------------------------------------------------
# data classes
@pytest.mark.parametrize("sq,skv", R.CLASS_SHAPES)
@pytest.mark.parametrize("name", R.CLASSES)
def test_data_classes(ops, name, sq, skv):
    case = _case(name, sq, skv, R.CLASS_HEADS)
    if name == "far_below":
        assert float(case[2].lse2.max()) < -130 and skv % 64 != 0      # a padded key's exp2(-lse) overflows in the dQ kernel's last tile
    if name == "far_above":
        assert float(case[2].lse2.min()) > 130
    got = _cpu(_run(ops, case))
    for n, t in zip(("dq", "dk", "dv"), got):
        assert bool(torch.isfinite(t.float()).all()), f"{name}: {n} has {int((~torch.isfinite(t.float())).sum())} non-finite elements"
    R.assert_within(got, case[2], f"CLASS {name} q={sq} kv={skv}", data_class=name)


def test_far_below_zero_control_without_padded_keys(ops):
    """The same scores with kv_len % 64 == 0: no padded key exists, so this separates the padding from the range of lse itself."""
    sq, skv = R.FAR_BELOW_CONTROL
    case = _case("far_below", sq, skv, R.CLASS_HEADS)
    assert float(case[2].lse2.max()) < -130 and skv % 64 == 0
    R.assert_within(_cpu(_run(ops, case)), case[2], f"CLASS far_below (control) q={sq} kv={skv}", data_class="far_below")


# ---------------------------------------------------------------------------------------------------------------------
# memory discipline, through the raw ABI
def _guarded(rows, cols, stride, rows_after):
    """A [rows + rows_after, stride] bf16 buffer filled with SENT; the kernel's output is its [:rows, :cols]."""
    buf = torch.empty((rows + rows_after, stride), dtype=BF, device="cuda")
    buf.view(torch.int16).fill_(SENT)
    return buf


def _guards_intact(buf, rows, cols):
    b = buf.view(torch.int16)
    return bool((b[:rows, cols:] == SENT).all()) and bool((b[rows:] == SENT).all())


def _workspace(lib, sq, skv, heads, tail=4096):
    n = int(lib.gf_flash_attn_bwd_workspace_bytes(sq, skv, heads))
    ws = torch.full((n + tail,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    return ws, n


def _raw(lib, q, k, v, o, dout, lse, ws, dq, dk, dv, heads, scale, over=None):
    """gf_flash_attn_bwd on tensors (pointers and row strides from them); `over` replaces single arguments by name."""
    ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    a = dict(q=ptr(q), k=ptr(k), v=ptr(v), o=ptr(o), dout=ptr(dout), lse=ptr(lse), workspace=ptr(ws), dq=ptr(dq), dk=ptr(dk), dv=ptr(dv),
             q_len=q.shape[0], kv_len=k.shape[0], heads=heads, head_dim=HD, q_stride=q.stride(0), k_stride=k.stride(0), v_stride=v.stride(0),
             o_stride=o.stride(0), do_stride=dout.stride(0), dq_stride=dq.stride(0), dk_stride=heads * HD if dk is None else dk.stride(0),
             dv_stride=heads * HD if dv is None else dv.stride(0), scale=float(scale), stream=torch.cuda.current_stream().cuda_stream)
    over = over or {}
    assert set(over) <= set(a), set(over) - set(a)
    a.update(over)
    rc = lib.gf_flash_attn_bwd(*a.values())
    torch.cuda.synchronize()
    return rc


MEM_CASES = [("std1", 97, 145, 2), ("std1", 129, 129, 3)]


@pytest.fixture(scope="module", params=MEM_CASES, ids=lambda c: f"q{c[1]}-kv{c[2]}-h{c[3]}")
def plain(request, ops, lib):
    """(case, device inputs, the plain contiguous call's dq, dk, dv) — also held to the bounds, once."""
    case = _case(*request.param)
    got = _run(ops, case)
    R.assert_within(_cpu(got), case[2], f"MEM plain {request.param}")
    return case, _dev(case), got


def test_inputs_inside_nan_filled_buffers(lib, plain):
    """q, k, v, o, dout and lse as the leading rows of longer NaN-filled buffers: the zero padding of a ragged tail comes from the
    descriptors, not from what lies behind the tensor."""
    case, (q, k, v, o, dout, lse), want = plain
    heads, D = case[2].heads, case[2].heads * HD
    qe, ke, ve, oe, de = (R.embed(t, 70, 0) for t in (q, k, v, o, dout))
    le = R.embed(lse, 70, 0)
    assert all(t.is_contiguous() for t in (qe, ke, ve, oe, de, le))
    ws, _ = _workspace(lib, q.shape[0], k.shape[0], heads)
    got = [torch.empty((n, D), dtype=BF, device="cuda") for n in (q.shape[0], k.shape[0], k.shape[0])]
    assert _raw(lib, qe, ke, ve, oe, de, le, ws, *got, heads, case[1]) == 0
    for name, a, b in zip(("dq", "dk", "dv"), got, want):
        assert _same(a, b), f"{name} changed with NaN rows behind the inputs"


def test_qkv_as_column_slices_of_a_fused_buffer_with_nan_gaps(ops, lib):
    """q | gap | k | gap | v in one [S, 3 D + 128] buffer whose gaps are NaN (q_len == kv_len, as the fused QKV projection gives them)."""
    case = _case(*MEM_CASES[1])
    q, k, v, o, dout, lse = _dev(case)
    want = _run(ops, case)
    heads, D, S = case[2].heads, case[2].heads * HD, q.shape[0]
    assert k.shape[0] == S
    fused = torch.full((S, 3 * D + 128), float("nan"), dtype=BF, device="cuda")
    views = []
    for i, t in enumerate((q, k, v)):
        views.append(fused[:, i * (D + 64): i * (D + 64) + D])
        views[-1].copy_(t)
    ws, _ = _workspace(lib, S, S, heads)
    got = [torch.empty((S, D), dtype=BF, device="cuda") for _ in range(3)]
    assert _raw(lib, *views, o, dout, lse, ws, *got, heads, case[1]) == 0
    for name, a, b in zip(("dq", "dk", "dv"), got, want):
        assert _same(a, b), f"{name} changed with q, k, v strided inside a NaN-padded fused buffer"


@pytest.mark.parametrize("wide", ["plus8", "times3"])
def test_strided_outputs_guards_and_workspace_tail(lib, plain, wide):
    """dq, dk, dv into guard-filled buffers with row strides heads*128 + 8 / 3 heads*128 and rows behind the end, the workspace exactly
    gf_flash_attn_bwd_workspace_bytes long with a guard tail: the same bits as the contiguous call, every guard element unchanged."""
    case, (q, k, v, o, dout, lse), want = plain
    heads, D = case[2].heads, case[2].heads * HD
    stride = D + 8 if wide == "plus8" else 3 * D
    bufs = [_guarded(n, D, stride, 3) for n in (q.shape[0], k.shape[0], k.shape[0])]
    outs = [b[:n, :D] for b, n in zip(bufs, (q.shape[0], k.shape[0], k.shape[0]))]
    ws, n_ws = _workspace(lib, q.shape[0], k.shape[0], heads)
    assert _raw(lib, q, k, v, o, dout, lse, ws, *outs, heads, case[1]) == 0
    for name, buf, out, b in zip(("dq", "dk", "dv"), bufs, outs, want):
        assert _same(out, b), f"{name} differs at row stride {stride}"
        assert _guards_intact(buf, out.shape[0], D), f"{name}: a guard element behind the rows or beside the columns was written"
    assert bool((ws[n_ws:] == 0xA5).all()), "the workspace was overrun"


def test_dq_alone_and_determinism(lib, plain):
    """dk = dv = NULL: the same dq bits, guard-filled dk / dv buffers (never passed) untouched; and a second full run gives the same bits
    (no atomics anywhere)."""
    case, (q, k, v, o, dout, lse), want = plain
    heads, D = case[2].heads, case[2].heads * HD
    dq = torch.empty((q.shape[0], D), dtype=BF, device="cuda")
    spare = [_guarded(k.shape[0], D, D, 0) for _ in range(2)]
    ws, n_ws = _workspace(lib, q.shape[0], k.shape[0], heads)
    assert _raw(lib, q, k, v, o, dout, lse, ws, dq, None, None, heads, case[1]) == 0
    assert _same(dq, want[0]), "dq differs when dk and dv are not asked for"
    assert all(bool((s.view(torch.int16) == SENT).all()) for s in spare) and bool((ws[n_ws:] == 0xA5).all())
    again = [torch.empty_like(t) for t in want]
    assert _raw(lib, q, k, v, o, dout, lse, ws, *again, heads, case[1]) == 0
    for name, a, b in zip(("dq", "dk", "dv"), again, want):
        assert _same(a, b), f"{name}: two runs differ"


# ---------------------------------------------------------------------------------------------------------------------
# refusals
REFUSALS = {
    "head_dim_64": (dict(head_dim=64), GF_ERR_UNSUPPORTED, "head_dim=64 unsupported"),
    "stride_not_multiple_of_8": (dict(k_stride=2 * HD + 4), GF_ERR_INVALID_ARG, "strides must cover heads*128 and be multiples of 8"),
    "stride_below_heads_x_128": (dict(dv_stride=2 * HD - 8), GF_ERR_INVALID_ARG, "strides must cover heads*128 and be multiples of 8"),
    "pointer_off_by_8_bytes": ("v+8", GF_ERR_INVALID_ARG, "16-byte alignment required"),
    "dk_without_dv": (dict(dv=None), GF_ERR_INVALID_ARG, "dk and dv may be NULL together"),
    "q_len_0": (dict(q_len=0), GF_ERR_INVALID_ARG, "bad lengths q=0"),
    "sequence_of_4_gib": (dict(q_stride=((1 << 31) // (40 + 64) + 8) // 8 * 8), GF_ERR_INVALID_ARG, "must stay below 4 GiB"),
}


@pytest.mark.parametrize("which", list(REFUSALS))
def test_refusals_leave_outputs_and_workspace_untouched(lib, which):
    """Each refusal returns the documented code and message before anything is launched: the guard-filled outputs and the workspace are
    as they were.  (The 4 GiB refusal is asked for with a huge row stride on a 40-row tensor: nothing is read.)"""
    over, code, msg = REFUSALS[which]
    sq, skv, heads = 40, 50, 2
    case = _case("std1", sq, skv, heads)
    q, k, v, o, dout, lse = _dev(case)
    if over == "v+8":
        over = dict(v=v.data_ptr() + 8)
    if "q_stride" in over:
        assert over["q_stride"] % 8 == 0 and (sq + 64) * over["q_stride"] * 2 >= (1 << 32) > (sq + 64) * (over["q_stride"] - 8) * 2
    outs = [_guarded(n, heads * HD, heads * HD, 0) for n in (sq, skv, skv)]
    ws, _ = _workspace(lib, sq, skv, heads, tail=0)
    rc = _raw(lib, q, k, v, o, dout, lse, ws, *outs, heads, case[1], over)
    text = lib.gf_last_error().decode()
    assert rc == code and msg in text, (rc, text)
    assert all(bool((t.view(torch.int16) == SENT).all()) for t in outs), "a refused call wrote to an output"
    assert bool((ws == 0xA5).all()), "a refused call wrote to the workspace"
    # and the same operands are accepted once the argument is right
    assert _raw(lib, q, k, v, o, dout, lse, ws, *outs, heads, case[1]) == 0
    R.assert_within(_cpu(outs), case[2], f"REFUSAL {which}: the accepted call")
