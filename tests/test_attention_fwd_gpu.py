"""The attention forward (goal_force_amd/csrc/gf_attention.hip: kernel 2, and kernel 3 in its exact, fixed-maximum and block-sparse forms)
pinned element by element against the fp64 reference of tests/attention_fwd_refs.py at every tile edge, on the data classes where it can
go wrong, and with its memory discipline and refusals checked, all through the raw C ABI — so kernel 3 runs at 128 .. 513 keys, far
below the 2048 from which ops.flash_attn sends it a sequence.

Every O is held to      |got - ref| <= u |ref| + u W + 2^-16 rms(ref row)          (u = 2^-8; W: the helper's docstring)
every (row, head) to the row bar (error norm <= 1.25 x the worst ratio the kernel's fp32 restatement reaches over these very cases
against the predicted rounding noise), every lse to its own bound; tests/test_attention_fwd_refs_cpu.py shows on the CPU that the
right restatements pass all of it and which injected faults do not.  Each comparison prints what it measured (`pytest -s`).

Edges (head_dim 128): 64-key tiles in a pipeline of prologue, steady phases unrolled by two and a tail — one tile (kernel 2), two
tiles (no steady phase), odd and even counts; the last tile's residue at the 16-key MFMA and 32-key lane-half / V^T-group boundaries;
32-query waves and 256-query workgroups; the XCD-ordered (head, block) decode at heads % 8 == 0.
"""
import pytest
import torch

import attention_fwd_refs as R
import attn_fixed_max_cases as fc

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
HD = R.HD
SENT = 0x5A5A                       # a finite bf16 bit pattern (1.5e16) no output here comes near
SENT_F, SENT_I = 1.25e30, 0x5A5A5A5A
GF_ERR_INVALID_ARG, GF_ERR_UNSUPPORTED = -1, -2
K2_ENTRIES = ("gf_flash_attn_fwd", "gf_flash_attn_fwd_lse", "gf_flash_attn_fwd_lastmult", "gf_flash_attn_fwd_vt")
K3_ENTRIES = ("gf_flash_attn_fwd_vt32", "gf_flash_attn_fwd_vt32_fm", "gf_flash_attn_fwd_vt32_sparse", "gf_flash_attn_fwd_vt32_sparse_fm")
_LENS = "q_len kv_len heads head_dim q_stride k_stride v_stride o_stride scale"
_LENS_VT = "q_len kv_len kv_pad heads head_dim q_stride k_stride o_stride scale stream"
_MAP = "row_ptr tile_idx head_map n_maps "
SIG = {
    "gf_flash_attn_fwd": f"q k v o {_LENS} stream",
    "gf_flash_attn_fwd_lse": f"q k v o lse {_LENS} stream",
    "gf_flash_attn_fwd_lastmult": f"q k v o {_LENS} mult stream",
    "gf_flash_attn_fwd_vt": f"q k vt o lse {_LENS_VT}",
    "gf_flash_attn_fwd_vt32": f"q k vt o lse {_LENS_VT}",
    "gf_flash_attn_fwd_vt32_fm": f"q k vt o lse flags {_LENS_VT}",
    "gf_flash_attn_fwd_vt32_sparse": f"q k vt o lse {_MAP}{_LENS_VT}",
    "gf_flash_attn_fwd_vt32_sparse_fm": f"q k vt o lse flags {_MAP}{_LENS_VT}",
    "gf_transpose_v": "v v_stride vt kv_len kv_pad heads stream",
    "gf_transpose_v32": "v v_stride vt kv_len kv_pad heads stream",
}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from goal_force_amd import ops as _ops
    assert _ops.lib_option("attn_fixed_max") == 1, "the fixed-maximum path is the default"
    return _ops


@pytest.fixture(scope="module")
def lib(ops):
    return ops._lib.load()


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


_CACHE = {}


def _case(name, sq, skv, heads, mult=1, mp=None):
    """((q, k, v) on the CPU, scale, maps, reference): computed once per case and left unchanged."""
    key = (name, sq, skv, heads, mult, mp)
    if key not in _CACHE:
        q, k, v, scale = R.case_inputs(name, sq, skv, heads)
        maps = sel = None
        if mp is not None:
            maps = R.sparse_map(mp, sq, skv, heads)
            sel = R.selection(*maps, heads, sq, skv)
        _CACHE[key] = ((q, k, v), scale, maps, R.attn_ref(q, k, v, heads, scale, mult, sel))
    return _CACHE[key]


def _pad(skv):
    return -(-skv // 64) * 64


def _ptr(t):
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def _raw(lib, entry, a, over=None):
    """`entry` with the arguments its signature names taken from the dict `a` (`over` replaces single ones); synchronises."""
    a = dict(a)
    a.update(over or {})
    assert set(over or {}) <= set(SIG[entry].split()), (entry, over)
    rc = getattr(lib, entry)(*[_ptr(a[n]) if n in ("q", "k", "v", "vt", "o", "lse", "flags", "row_ptr", "tile_idx", "head_map") else a[n]
                               for n in SIG[entry].split()])
    torch.cuda.synchronize()
    return rc


def _args(q, k, v, o, heads, scale, **more):
    a = dict(q=q, k=k, v=v, o=o, lse=None, flags=None, vt=None, q_len=q.shape[0], kv_len=k.shape[0], kv_pad=_pad(k.shape[0]), heads=heads,
             head_dim=HD, q_stride=q.stride(0), k_stride=k.stride(0), v_stride=v.stride(0), o_stride=o.stride(0), scale=float(scale), mult=1.0,
             row_ptr=None, tile_idx=None, head_map=None, n_maps=0, stream=torch.cuda.current_stream().cuda_stream)
    a.update(more)
    return a


def _transpose(lib, v, heads, group, check=True):
    """V^T of gf_transpose_v (group 16) / gf_transpose_v32 (group 32) in a NaN-filled buffer with a guard tail; with `check`, the pad
    columns are zero, the rest is the documented permutation and the tail is intact."""
    skv, kvp = v.shape[0], _pad(v.shape[0])
    n = heads * HD * kvp
    buf = torch.full((n + 256,), float("nan"), dtype=BF, device="cuda")
    buf[n:].view(torch.int16).fill_(SENT)
    entry = "gf_transpose_v" if group == 16 else "gf_transpose_v32"
    assert _raw(lib, entry, dict(v=v, v_stride=v.stride(0), vt=buf, kv_len=skv, kv_pad=kvp, heads=heads,
                                 stream=torch.cuda.current_stream().cuda_stream)) == 0, lib.gf_last_error()
    if check:
        vt3 = buf[:n].view(heads, HD, kvp).cpu()
        assert bool((buf[n:].view(torch.int16) == SENT).all()), f"{entry} wrote behind heads*128*kv_pad"
        vpad = torch.zeros((kvp, heads, HD), dtype=BF)
        vpad[:skv] = v.cpu().reshape(skv, heads, HD)
        pos = R.vt_positions(kvp, group)
        assert torch.equal(vt3.view(torch.int16), vpad[pos].permute(1, 2, 0).contiguous().view(torch.int16)), \
            f"{entry}: not the documented permutation with zero pad columns (kv_len {skv})"
    return buf[:n]


def _maps_dev(maps):
    lists, hm = maps
    rp, ti = R.csr(lists)
    return dict(row_ptr=rp.cuda(), tile_idx=ti.cuda(), head_map=None if hm is None else torch.tensor(hm, dtype=torch.int32).cuda(),
                n_maps=len(lists))


def _run(lib, entry, case, want_lse=True, maps=None, dev=None, heads=None, **over):
    """(o, lse or None, flags or None) on the GPU of `entry` on the case's operands (contiguous; `dev`: these device tensors in their
    place, `heads`: their head count where it is not the case's)."""
    (q, k, v), scale, case_maps, ref = case
    q, k, v = dev if dev is not None else (t.cuda() for t in (q, k, v))
    sq, heads = q.shape[0], heads or ref.heads
    o = torch.empty((sq, heads * HD), dtype=BF, device="cuda")
    o.view(torch.int16).fill_(SENT)
    a = _args(q, k, v, o, heads, scale, mult=float(ref.mult))
    if "lse" in SIG[entry].split() and want_lse:
        a["lse"] = torch.full((sq, heads), SENT_F, dtype=torch.float32, device="cuda")
    if "flags" in SIG[entry].split():
        a["flags"] = torch.full((heads, -(-sq // 256), 8), SENT_I, dtype=torch.int32, device="cuda")
    if "vt" in SIG[entry].split():
        a["vt"] = _transpose(lib, v, heads, 16 if entry == "gf_flash_attn_fwd_vt" else 32, check=False)
    if "row_ptr" in SIG[entry].split():
        a.update(_maps_dev(maps or case_maps))
    assert _raw(lib, entry, a, over) == 0, lib.gf_last_error().decode()
    return o, a["lse"], a["flags"]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _within(o, lse, case, kind, what):
    return R.assert_within(o.cpu(), None if lse is None else lse.cpu(), case[3], kind, what)


# ---------------------------------------------------------------------------------------------------------------------
# tile edges
@pytest.mark.parametrize("sq,skv", R.K2_PAIRS)
def test_kernel2_tile_edges(lib, sq, skv):
    """gf_flash_attn_fwd_lse through the bounds; gf_flash_attn_fwd the same O bits; gf_transpose_v's layout, and gf_flash_attn_fwd_vt on
    it the same O and lse bits as the plain path."""
    for heads in R.TILE_HEADS:
        case = _case("std1", sq, skv, heads)
        dev = tuple(t.cuda() for t in case[0])
        o, lse, _ = _run(lib, "gf_flash_attn_fwd_lse", case, dev=dev)
        _within(o, lse, case, "k2", f"K2 q={sq} kv={skv} heads={heads}")
        assert _same(_run(lib, "gf_flash_attn_fwd", case, dev=dev)[0], o), "gf_flash_attn_fwd differs from gf_flash_attn_fwd_lse"
        _transpose(lib, dev[2], heads, 16)
        o_vt, lse_vt, _ = _run(lib, "gf_flash_attn_fwd_vt", case, dev=dev)
        assert _same(o_vt, o) and _same(lse_vt, lse), "the V^T path differs from the plain path"
        o_vt0, none, _ = _run(lib, "gf_flash_attn_fwd_vt", case, want_lse=False, dev=dev)
        assert none is None and _same(o_vt0, o)


@pytest.mark.parametrize("sq,skv", R.K3_PAIRS)
def test_kernel3_tile_edges(ops, lib, sq, skv):
    """gf_flash_attn_fwd_vt32 and _vt32_fm through the bounds (no flag set); gf_transpose_v32's layout; a full map is dense bit for bit,
    in both modes; with attn_fixed_max off _fm is the exact entry point bit for bit and its flags are all zero."""
    nt, nb = -(-skv // 64), -(-sq // 256)
    full = ([[list(range(nt)) for _ in range(nb)]], None)
    for name, heads in R.K3_EDGE_CLASSES:      # std1; prescaled (the sharper bound); far_below (where a mask off by one cannot hide)
        case = _case(name, sq, skv, heads)
        dev = tuple(t.cuda() for t in case[0])
        _transpose(lib, dev[2], heads, 32)
        o, lse, _ = _run(lib, "gf_flash_attn_fwd_vt32", case, dev=dev)
        _within(o, lse, case, "k3", f"K3 {name} q={sq} kv={skv} heads={heads}")
        o_fm, lse_fm, flags = _run(lib, "gf_flash_attn_fwd_vt32_fm", case, dev=dev)
        assert int(flags.count_nonzero()) == 0, flags.tolist()
        _within(o_fm, lse_fm, case, "k3fm", f"K3 fixed maximum {name} q={sq} kv={skv} heads={heads}")
        o_s, lse_s, _ = _run(lib, "gf_flash_attn_fwd_vt32_sparse", case, maps=full, dev=dev)
        assert _same(o_s, o) and _same(lse_s, lse), "a full map differs from the dense entry point"
        o_sf, lse_sf, flags_s = _run(lib, "gf_flash_attn_fwd_vt32_sparse_fm", case, maps=full, dev=dev)
        assert _same(o_sf, o_fm) and _same(lse_sf, lse_fm) and int(flags_s.count_nonzero()) == 0
        with ops.options(attn_fixed_max=0):
            for entry, kw in (("gf_flash_attn_fwd_vt32_fm", {}), ("gf_flash_attn_fwd_vt32_sparse_fm", dict(maps=full))):
                o_off, lse_off, flags_off = _run(lib, entry, case, dev=dev, **kw)
                assert _same(o_off, o) and _same(lse_off, lse) and int(flags_off.count_nonzero()) == 0, f"{entry} with the option off"
        assert ops.lib_option("attn_fixed_max") == 1


# ---------------------------------------------------------------------------------------------------------------------
# the XCD-ordered grid
def _head_alone(lib, entry, case, h):
    c = slice(h * HD, (h + 1) * HD)
    return _run(lib, entry, case, dev=tuple(t[:, c].cuda().contiguous() for t in case[0]), heads=1)


@pytest.mark.parametrize("kind,sq,skv,heads", [("k2", *c) for c in R.K2_XCD] + [("k3", *c) for c in R.K3_XCD] + [("k3fm", *c) for c in R.K3_XCD])
def test_xcd_ordered_grid(lib, kind, sq, skv, heads):
    """heads 8 and 16, each with two and with three query blocks: per element against fp64, and bit-identical, head by head, to that head run
    alone — which pins the (head, block) decode exactly."""
    entry = {"k2": "gf_flash_attn_fwd_lse", "k3": "gf_flash_attn_fwd_vt32", "k3fm": "gf_flash_attn_fwd_vt32_fm"}[kind]
    case = _case("std1", sq, skv, heads)
    o, lse, _ = _run(lib, entry, case)
    _within(o, lse, case, kind, f"XCD {kind} q={sq} kv={skv} heads={heads}")
    for h in range(heads):
        o1, lse1, _ = _head_alone(lib, entry, case, h)
        assert _same(o[:, h * HD:(h + 1) * HD], o1) and _same(lse[:, h:h + 1], lse1), f"head {h} of {heads} differs from the head run alone"


# ---------------------------------------------------------------------------------------------------------------------
# data classes
CLASS_ENTRY = {"k2": "gf_flash_attn_fwd_lse", "k3": "gf_flash_attn_fwd_vt32", "k3fm": "gf_flash_attn_fwd_vt32_fm"}


def _class(lib, kind, name, shape):
    case = _case(name, *shape, R.CLASS_HEADS)
    o, lse, flags = _run(lib, CLASS_ENTRY[kind], case)
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse).all()), f"{name}: non-finite o or lse"
    if flags is not None:        # no class here rises more than 60 log2 units above tile 0: nothing to repair
        assert int(flags.count_nonzero()) == 0, (name, flags.tolist())
    _within(o, lse, case, kind, f"CLASS {kind} {name} q={shape[0]} kv={shape[1]}")
    return case, o, lse


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("name", R.CLASSES)
def test_data_classes(lib, kind, name):
    case, o, lse = _class(lib, kind, name, R.CLASS_SHAPE)
    ref = case[3]
    if name == "far_below":
        assert float(ref.lse2.max()) < -180 and R.CLASS_SHAPE[1] % 64 != 0      # the ragged tile's zero keys score 0: 200 above the real ones
    if name == "far_above":
        assert float(ref.lse2.min()) > 180
    if name == "v_const" and kind != "k2":                                      # kernel 3 sums the p it multiplies: the row itself, exactly
        assert _same(o, case[0][2][:1].expand(o.shape[0], -1).cuda())


@pytest.mark.parametrize("kind", R.KINDS)
def test_far_below_zero_control_without_a_ragged_tile(lib, kind):
    assert R.FAR_BELOW_CONTROL[1] % 64 == 0
    _class(lib, kind, "far_below", R.FAR_BELOW_CONTROL)


# ---------------------------------------------------------------------------------------------------------------------
# the multiplicity of the last key
@pytest.mark.parametrize("n", R.MULT_KV)
@pytest.mark.parametrize("m", R.MULTS)
def test_last_key_multiplicity(lib, m, n):
    """gf_flash_attn_fwd_lastmult against the attention over the keys written out; multiplicity 1 is gf_flash_attn_fwd bit for bit."""
    case = _case("std1", R.MULT_Q, n, R.MULT_HEADS, m)
    o, _, _ = _run(lib, "gf_flash_attn_fwd_lastmult", case)
    _within(o, None, case, "k2", f"LASTMULT m={m} n={n}")
    if m == 1:
        assert _same(o, _run(lib, "gf_flash_attn_fwd", case)[0])


# ---------------------------------------------------------------------------------------------------------------------
# block-sparse
@pytest.mark.parametrize("fm", [False, True], ids=["exact", "fixed_max"])
@pytest.mark.parametrize("name", R.SPARSE_MAPS)
def test_sparse_maps(lib, name, fm):
    """Against the fp64 softmax over the selected keys: a full map, a random ascending one, lists that end in and that skip the ragged
    tile, a one-tile list, two maps behind a head_map."""
    case = _case("std1", *R.SPARSE_SHAPE, 1, name)
    o, lse, flags = _run(lib, "gf_flash_attn_fwd_vt32_sparse_fm" if fm else "gf_flash_attn_fwd_vt32_sparse", case)
    assert flags is None or int(flags.count_nonzero()) == 0
    _within(o, lse, case, "k3fm" if fm else "k3", f"SPARSE {name} {'fixed maximum' if fm else 'exact'}")


# ---------------------------------------------------------------------------------------------------------------------
# the fixed maximum's overflow and repair
@pytest.mark.parametrize("name", list(R.OVERFLOW))
def test_overflow_is_flagged_in_one_workgroup_and_repaired(lib, name):
    """One key OVERFLOW_RISE log2 units above tile 0 for ONE query: flags are set in the workgroup of that row alone, the row's wave is
    among them, the workgroup's rows are the exact entry point's bits and the whole result is within the bounds."""
    sq, skv = R.CLASS_SHAPE
    case = _case(name, sq, skv, R.CLASS_HEADS)
    s = fc.scores(case[0][0], case[0][1], R.RISE_HEAD)[R.RISE_ROW]
    assert float(s[R.RISE_KEYS[R.OVERFLOW[name]]] - s[:64].max()) >= 130
    o, lse, flags = _run(lib, "gf_flash_attn_fwd_vt32_fm", case)
    flags = flags.cpu()
    block, wave = R.RISE_ROW // 256, (R.RISE_ROW % 256) // 32
    assert int(flags[R.RISE_HEAD, block, wave]) == 1, flags.tolist()
    flags[R.RISE_HEAD, block] = 0
    assert int(flags.count_nonzero()) == 0, "a flag outside the workgroup of the rise row"
    _within(o, lse, case, "k3", f"OVERFLOW {name}")
    o_x, lse_x, _ = _run(lib, "gf_flash_attn_fwd_vt32", case)
    rows, cols = slice(256 * block, sq), slice(HD * R.RISE_HEAD, HD * R.RISE_HEAD + HD)
    assert _same(o[rows, cols], o_x[rows, cols]) and _same(lse[rows, R.RISE_HEAD], lse_x[rows, R.RISE_HEAD])


# ---------------------------------------------------------------------------------------------------------------------
# surroundings
def _guarded(rows, cols, stride, rows_after=3):
    buf = torch.empty((rows + rows_after, stride), dtype=BF, device="cuda")
    buf.view(torch.int16).fill_(SENT)
    return buf


def _between(rows, cols, dtype, fill):
    """A [rows, cols] contiguous view with two guard rows before and after it."""
    buf = torch.full((rows + 4, cols), fill, dtype=dtype, device="cuda")
    return buf, buf[2:2 + rows]


# (the kernel-2 shapes are attention_fwd_refs.MEM_CASES, the others class or sparse cases: all of them in all_cases())
SURROUND = [("gf_flash_attn_fwd_lse", "std1", 97, 145, 2, None), ("gf_flash_attn_fwd_vt", "std1", 97, 145, 2, None),
            ("gf_flash_attn_fwd_lastmult", "std1", 65, 97, 2, None), ("gf_flash_attn_fwd_vt32", "far_below", 289, 161, 2, None),
            ("gf_flash_attn_fwd_vt32_fm", "std1", 289, 161, 2, None), ("gf_flash_attn_fwd_vt32_sparse", "std1", *R.SPARSE_SHAPE, "random"),
            ("gf_flash_attn_fwd_vt32_sparse_fm", "std1", *R.SPARSE_SHAPE, "two_maps")]


@pytest.mark.parametrize("o_extra", [4, 8])
@pytest.mark.parametrize("entry,name,sq,skv,heads,mp", SURROUND, ids=[s[0][3:] for s in SURROUND])
def test_nan_surroundings_and_guards(lib, entry, name, sq, skv, heads, mp, o_extra):
    """q, k and v are slices of NaN-filled parents (rows behind, columns on both sides, row strides above heads*128), O goes into a
    guard-filled parent with o_stride = heads*128 + 4 / + 8, lse and flags sit between guards: the same bits as the contiguous call
    (which is inside the bounds), every guard intact; and q_len == 0 returns OK and touches nothing."""
    case = _case(name, sq, skv, heads, 3 if "lastmult" in entry else 1, mp)
    kind = "k2" if entry in K2_ENTRIES else ("k3fm" if entry.endswith("_fm") else "k3")
    want_o, want_lse, want_flags = _run(lib, entry, case)
    _within(want_o, want_lse, case, kind, f"SURROUND {entry} (contiguous)")
    D = heads * HD
    q, k, v = (R.embed(t.cuda(), 70, 8, 16) for t in case[0])
    assert all(t.stride(0) == D + 24 and t.data_ptr() % 16 == 0 and not t.is_contiguous() for t in (q, k, v))
    obuf = _guarded(sq, D, D + o_extra)
    a = _args(q, k, v, obuf[:sq, :D], heads, case[1], mult=float(case[3].mult))
    names = SIG[entry].split()
    lbuf = fbuf = None
    if "lse" in names:
        lbuf, a["lse"] = _between(sq, heads, torch.float32, SENT_F)
    if "flags" in names:
        fbuf, a["flags"] = _between(heads * -(-sq // 256), 8, torch.int32, SENT_I)
    if "vt" in names:
        a["vt"] = _transpose(lib, v, heads, 16 if entry == "gf_flash_attn_fwd_vt" else 32)      # (from the strided v)
    if "row_ptr" in names:
        a.update(_maps_dev(case[2]))

    def guards_intact():
        ob = obuf.view(torch.int16)
        ok = bool((ob[:sq, D:] == SENT).all()) and bool((ob[sq:] == SENT).all())
        if lbuf is not None:
            ok = ok and bool((lbuf[:2] == SENT_F).all()) and bool((lbuf[-2:] == SENT_F).all())
        if fbuf is not None:
            ok = ok and bool((fbuf[:2] == SENT_I).all()) and bool((fbuf[-2:] == SENT_I).all())
        return ok

    assert _raw(lib, entry, a, dict(q_len=0)) == 0, lib.gf_last_error().decode()
    assert bool((obuf.view(torch.int16) == SENT).all()) and guards_intact(), "q_len == 0 wrote something"
    assert lbuf is None or bool((lbuf == SENT_F).all())
    assert fbuf is None or bool((fbuf == SENT_I).all())
    assert _raw(lib, entry, a) == 0, lib.gf_last_error().decode()
    assert guards_intact(), "a guard element was written"
    assert _same(obuf[:sq, :D], want_o), f"O changed inside NaN surroundings at o_stride {D + o_extra}"
    if want_lse is not None:
        assert _same(a["lse"], want_lse), "lse changed inside NaN surroundings"
    if want_flags is not None:
        assert torch.equal(a["flags"].view(-1), want_flags.view(-1))


# ---------------------------------------------------------------------------------------------------------------------
# refusals
def _huge_stride(kv_len):
    s = ((1 << 31) // (kv_len + 64) + 8) // 8 * 8
    assert (kv_len + 64) * s >= (1 << 31) > (kv_len + 64) * (s - 8)
    return s


def _refusals(entry, heads, kv_len):
    """{name: (overrides, code, message)} of every refusal of `entry`."""
    D, bad = heads * HD, GF_ERR_INVALID_ARG
    if entry.startswith("gf_transpose"):
        msg = f"{entry}: kv_pad must be a multiple of 64 covering kv_len; v_stride must cover heads*128"
        return {"null_v": (dict(v=None), bad, f"{entry}: null pointer"), "null_vt": (dict(vt=None), bad, f"{entry}: null pointer"),
                "kv_len_0": (dict(kv_len=0), bad, msg), "heads_0": (dict(heads=0), bad, msg),
                "kv_pad_short": (dict(kv_pad=_pad(kv_len) - 64), bad, msg), "kv_pad_not_x64": (dict(kv_pad=_pad(kv_len) + 32), bad, msg),
                "v_stride_not_x8": (dict(v_stride=D + 4), bad, msg), "v_stride_short": (dict(v_stride=D - 8), bad, msg),
                "v_off_by_8_bytes": ("v+8", bad, f"{entry}: 16-byte alignment required"),
                "vt_off_by_8_bytes": ("vt+8", bad, f"{entry}: 16-byte alignment required"),
                "kv_pad_2_31": (dict(kv_pad=(1 << 31) // D), bad, f"{entry}: heads*128*kv_pad must stay below 2^31 elements")}
    k3 = entry in K3_ENTRIES
    fn = entry if k3 else "gf_flash_attn_fwd"
    strides = f"{fn}: strides must cover heads*128 and be multiples of 8"
    out = {
        "null_q": (dict(q=None), bad, f"{fn}: null pointer"), "null_o": (dict(o=None), bad, f"{fn}: null pointer"),
        "head_dim_64": (dict(head_dim=64), GF_ERR_UNSUPPORTED, f"{fn}: head_dim=64 unsupported"),
        "heads_0": (dict(heads=0), bad, f"{fn}: bad lengths"), "q_len_negative": (dict(q_len=-1), bad, f"{fn}: bad lengths"),
        "q_stride_not_x8": (dict(q_stride=D + 4), bad, strides), "k_stride_short": (dict(k_stride=D - 8), bad, strides),
        "o_stride_not_x4": (dict(o_stride=D + 2), bad, strides), "o_stride_short": (dict(o_stride=D - 4), bad, strides),
        "q_off_by_8_bytes": ("q+8", bad, f"{fn}: 16-byte alignment required"), "o_off_by_8_bytes": ("o+8", bad, f"{fn}: 16-byte alignment required"),
        "k_stride_2_31": (dict(k_stride=_huge_stride(kv_len)), bad, f"{fn}: kv_len*stride must stay below 2^31 elements"),
    }
    if k3:
        vtmsg = f"{fn}: bad V^T buffer"
        out.update({"null_vt": (dict(vt=None), bad, f"{fn}: null pointer"), "kv_len_127": (dict(kv_len=127, kv_pad=128), bad, f"{fn}: bad lengths q="),
                    "q_len_2_30": (dict(q_len=1 << 30), bad, "(kv_len >= 128)"),
                    "kv_pad_short": (dict(kv_pad=_pad(kv_len) - 64), bad, vtmsg), "kv_pad_not_x64": (dict(kv_pad=_pad(kv_len) + 32), bad, vtmsg),
                    "kv_pad_2_31": (dict(kv_pad=(1 << 31) // D), bad, vtmsg), "vt_off_by_8_bytes": ("vt+8", bad, f"{fn}: 16-byte alignment required")})
        if "sparse" in entry:
            out.update({"null_row_ptr": (dict(row_ptr=None), bad, f"{entry}: null map pointer"), "null_tile_idx": (dict(tile_idx=None), bad, f"{entry}: null map pointer"),
                        "n_maps_0": (dict(n_maps=0), bad, f"{entry}: n_maps=0")})
        if entry.endswith("_fm"):
            out.update({"null_flags": (dict(flags=None), bad, f"{entry}: null or misaligned flags workspace"),
                        "flags_off_by_2_bytes": ("flags+2", bad, f"{entry}: null or misaligned flags workspace")})
    else:
        out.update({"kv_len_0": (dict(kv_len=0, kv_pad=0), bad, f"{fn}: bad lengths q="), "q_len_2_30": (dict(q_len=1 << 30), bad, f"{fn}: sequence too long")})
        if entry == "gf_flash_attn_fwd_vt":
            vtmsg = "gf_flash_attn_fwd_vt: bad V^T buffer"
            out.update({"null_vt": (dict(vt=None), bad, vtmsg), "kv_pad_short": (dict(kv_pad=_pad(kv_len) - 64), bad, vtmsg),
                        "kv_pad_not_x64": (dict(kv_pad=_pad(kv_len) + 32), bad, vtmsg), "vt_off_by_8_bytes": ("vt+8", bad, vtmsg),
                        "kv_pad_2_31": (dict(kv_pad=(1 << 31) // D), bad, "gf_flash_attn_fwd_vt: heads*128*kv_pad must stay below 2^31 elements")})
        else:
            out.update({"null_v": (dict(v=None), bad, f"{fn}: null pointer"), "v_stride_not_x8": (dict(v_stride=D + 4), bad, strides),
                        "v_off_by_8_bytes": ("v+8", bad, f"{fn}: 16-byte alignment required"),
                        "v_stride_2_31": (dict(v_stride=_huge_stride(kv_len)), bad, f"{fn}: kv_len*stride must stay below 2^31 elements")})
        if entry == "gf_flash_attn_fwd_lse":
            out["null_lse"] = (dict(lse=None), bad, "gf_flash_attn_fwd_lse: null lse")
        if entry == "gf_flash_attn_fwd_lastmult":
            msg = "gf_flash_attn_fwd_lastmult: multiplicity >= 1, plain-V form only"
            out.update({"multiplicity_below_1": (dict(mult=0.5), bad, msg), "multiplicity_with_scale_0": (dict(mult=2.0, scale=0.0), bad, msg)})
    names = SIG[entry].split()           # (kv_pad rides along only where the entry point has one)
    return {w: (o if isinstance(o, str) else {n: x for n, x in o.items() if n in names}, c, m) for w, (o, c, m) in out.items()}


@pytest.mark.parametrize("entry", list(SIG), ids=[e[3:] for e in SIG])
def test_refusals_leave_every_output_untouched(lib, entry):
    """Every GF_CHECK_ARG and the GF_ERR_UNSUPPORTED of the entry point: the documented code, the message, and the guard-filled outputs
    (O, lse, flags, V^T for a transposer) as they were — nothing is launched.  Then the same operands are accepted."""
    sq, skv, heads = 40, 150, 2
    case = _case("std1", sq, skv, heads, 1, None)
    q, k, v = (t.cuda() for t in case[0])
    D, kvp = heads * HD, _pad(skv)
    o = _guarded(sq, D, D, 0)
    a = _args(q, k, v, o, heads, case[1])
    a["lse"] = torch.full((sq, heads), SENT_F, dtype=torch.float32, device="cuda")
    a["flags"] = torch.full((heads * 8 + 1,), SENT_I, dtype=torch.int32, device="cuda")
    transposer = entry.startswith("gf_transpose")
    if transposer:
        a["vt"] = _guarded(D, kvp, kvp, 0)
        outs = [a["vt"]]
    else:
        a["vt"] = _transpose(lib, v, heads, 16 if entry == "gf_flash_attn_fwd_vt" else 32, check=False)
        outs = [o]
    a.update(_maps_dev(([[[0, 2]]], None)))
    if entry == "gf_flash_attn_fwd_lastmult":
        a["mult"] = 2.0

    def untouched():
        return all(bool((t.view(torch.int16) == SENT).all()) for t in outs) and bool((a["lse"] == SENT_F).all()) and bool((a["flags"] == SENT_I).all())

    table = _refusals(entry, heads, skv)
    assert len(table) >= 10
    for which, (over, code, msg) in table.items():
        if isinstance(over, str):
            name, off = over.split("+")
            over = {name: a[name].data_ptr() + int(off)}
        rc = _raw(lib, entry, a, over)
        text = lib.gf_last_error().decode()
        assert rc == code and msg in text, (entry, which, rc, text)
        assert untouched(), f"{entry} refused ({which}) and still wrote to an output"
    assert _raw(lib, entry, a) == 0, lib.gf_last_error().decode()
    assert not untouched()
