"""gf_lora_grad per element through the raw C ABI (goal_force_amd/csrc/gf_lora_grad.hip).  The chain, the restatement, the bars and
the inputs are tests/lora_train_refs.py's; tests/test_lora_grad_refs_cpu.py shows that the fp32 restatement passes the bars on every
gauss input used here and that each stated fault does not.

The exact classes (selector: every output is a sum of named tokens' elements of one column; integers) with torch.equal on the bits,
gauss through gemm_refs' two bars with K = M.  The slab boundaries are read from gf_lora_grad_slabs / gf_lora_grad_slab_rows.  Every
call reads Y and T as strided views inside NaN-filled parents that go on for rows >= M, writes into a strided view inside a
sentinel-filled parent, and gets a workspace of exactly gf_lora_grad_workspace_bytes bytes with a sentinel guard behind it."""
import pytest
import torch

import gemm_refs as G
import lora_train_refs as T
from test_lora_gpu import GF_ERR_INVALID_ARG, SENT, Held, _bits, _err, _st

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CASES = T.grad_cases()
FIG = dict(n=0, share=0.0, worst=0.0)


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


def _p(x):
    return None if x is None else (x if isinstance(x, int) else x.data_ptr())


def _grad(lib, Y, ldy, Tm, ldt, out, ldo, M, C, rp, scale, transposed, ws):
    return lib.gf_lora_grad(_p(Y), ldy, _p(Tm), ldt, _p(out), ldo, M, C, rp, scale, transposed, _p(ws), _st())


class Workspace:
    """Exactly `nbytes` bytes at a 16-byte aligned address, NaN-filled (a partial the sum kernel reads without its slab having
    written it poisons the result), 256 sentinel bytes in front and behind."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.parent = torch.full((256 + nbytes + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        assert self.parent.data_ptr() % 16 == 0
        self.view = self.parent[256:256 + nbytes]
        if nbytes:
            self.view.view(torch.float32).fill_(float("nan"))

    def guards_intact(self):
        return bool((self.parent[:256] == 0x5A).all()) and bool((self.parent[256 + self.nbytes:] == 0x5A).all())


def _slabs(lib, M, C, rp):
    """The library's slab boundaries, held to the restatement the reference helpers use."""
    n, rows = lib.gf_lora_grad_slabs(M, C, rp), lib.gf_lora_grad_slab_rows(M, C, rp)
    bounds = [(s * rows, min(M, (s + 1) * rows)) for s in range(n)]
    assert bounds == T.slab_bounds(M, C), f"the slab rule moved: the library says {bounds}, tests/lora_train_refs.py {T.slab_bounds(M, C)}"
    return bounds


def _call_held(lib, d, extra_rows=3):
    """One call in guarded surroundings -> (result on the CPU, the out Held, the workspace).  The parents of Y and T carry
    `extra_rows` NaN rows behind row M - 1."""
    M, C = d["Y"].shape
    rp = d["T"].shape[1]
    nan = lambda r, c: torch.full((r, c), float("nan"), dtype=BF)          # noqa: E731
    Y = Held(torch.cat([d["Y"], nan(extra_rows, C)]), C + 8)
    Tm = Held(torch.cat([d["T"], nan(extra_rows, rp)]), rp + 16)
    rows, cols = (rp, C) if d["transposed"] else (C, rp)
    out = Held(torch.zeros((rows, cols), dtype=BF), cols + 24, fill="sentinel")
    out.view.view(torch.int16).fill_(SENT)                                  # every element of out must be WRITTEN
    ws = Workspace(lib.gf_lora_grad_workspace_bytes(M, C, rp))
    rc = _grad(lib, Y.view, Y.ld, Tm.view, Tm.ld, out.view, out.ld, M, C, rp, d["scale"], int(d["transposed"]), ws.view)
    torch.cuda.synchronize()
    assert rc == 0, _err(lib)
    assert out.guards_intact(), "gf_lora_grad wrote outside out (the ldo gap or behind it)"
    assert ws.guards_intact(), "gf_lora_grad wrote outside its workspace"
    assert Y.untouched() and Tm.untouched()
    return out.view.cpu(), out, ws


def _name(diff, d, bounds):
    """The first differing elements as (column of Y, rank column), and for the selector class the tokens that feed them with their slabs."""
    idx = torch.nonzero(diff.t() if d["transposed"] else diff)[:4].tolist()
    text = f"{int(diff.sum())} elements differ; first (column c, rank column j): {idx}"
    if "j" in d:
        for c, j in idx[:2]:
            toks = torch.nonzero(d["j"] == j).flatten().tolist()
            text += f"; out[{c}, {j}] sums tokens {[(m, next(s for s, (a, b) in enumerate(bounds) if a <= m < b)) for m in toks[:12]]} (token, slab) of column {c}"
    return text


def _check(lib, got, d, cls, what):
    M, C = d["Y"].shape
    rp, r = d["T"].shape[1], d["rank"]
    ref = T.grad_ref(d)
    bounds = _slabs(lib, M, C, rp)
    pad = got[r:] if d["transposed"] else got[:, r:]
    assert not bool(_bits(pad).any()), f"{what}: the rank's padding (columns {r} .. {rp - 1}) must be +0 bit for bit"
    if cls == "gauss":
        j = G.assert_pinned(got, ref, M, what)
        FIG.update(n=FIG["n"] + 1, share=max(FIG["share"], j["share"]), worst=max(FIG["worst"], j["worst"]))
        return
    diff = _bits(got) != _bits(ref.out.to(BF))
    print(f"PIN {what}: equal to the chain {not bool(diff.any())} ({len(bounds)} slabs)")
    assert not bool(diff.any()), f"{what}: exact operands, so any difference is a fault: {_name(diff, d, bounds)}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "M{}-C{}-rp{}-r{}-s{}-{}".format(*c[:5], "T" if c[5] else "N"))
def test_token_and_column_edges_three_classes(lib, case):
    M, C, rp, r, scale, tr = case
    for cls in T.CLASSES:
        d = T.grad_inputs(cls, M, C, rp, r, scale, tr)
        got, _, _ = _call_held(lib, d)
        _check(lib, got, d, cls, f"lora_grad {cls} {case}")


def test_both_orientations_hold_the_same_values_and_two_calls_the_same_bits(lib):
    for case in CASES[-4:]:
        M, C, rp, r, scale, _ = case
        d = T.grad_inputs("gauss", M, C, rp, r, scale, False)
        a, _, _ = _call_held(lib, d)
        b, _, _ = _call_held(lib, d, extra_rows=70)
        assert torch.equal(_bits(a), _bits(b)), f"{case}: two calls on the same operands differ"
        t, _, _ = _call_held(lib, dict(d, transposed=True))
        assert torch.equal(_bits(t), _bits(a.t().contiguous())), f"{case}: the transposed store holds other values"


def test_slab_cases_are_what_they_are_named(lib):
    two, last = CASES[len(T.GRAD_M)], CASES[len(T.GRAD_M) + 1]
    assert len(_slabs(lib, two[0], two[1], two[2])) == 2 and len(_slabs(lib, two[0] - 1, two[1], two[2])) == 1
    b = _slabs(lib, last[0], last[1], last[2])
    assert len(b) >= 3 and b[-1][1] - b[-1][0] == 1
    # the production shapes fill the device
    for C in (5120, 13824):
        assert 1024 <= lib.gf_lora_grad_slabs(32760, C, 32) * -(-C // 64) <= 1280


def test_no_tokens_writes_plus_zero(lib):
    for tr in (False, True):
        d = T.grad_inputs("integers", 0, 72, 64, 4, -1.3, tr)
        assert lib.gf_lora_grad_workspace_bytes(0, 72, 64) == 0 and lib.gf_lora_grad_slabs(0, 72, 64) == 0
        got, out, _ = _call_held(lib, d)
        assert not bool(_bits(got).any())
        # a null workspace is taken when no byte is asked for
        out.view.view(torch.int16).fill_(SENT)
        Y, Tm = torch.empty((1, 72), dtype=BF, device="cuda"), torch.empty((1, 64), dtype=BF, device="cuda")
        assert _grad(lib, Y, 72, Tm, 64, out.view, out.ld, 0, 72, 64, 1.0, int(tr), None) == 0, _err(lib)
        torch.cuda.synchronize()
        assert not bool(_bits(out.view.cpu()).any()) and out.guards_intact()


def test_refusals_leave_out_untouched(ops, lib):
    d = T.grad_inputs("integers", 65, 72, 64, 4, 1.0)
    Y, Tm = Held(d["Y"], 80), Held(d["T"], 72)
    out = Held(torch.zeros((72, 64), dtype=BF), 72, fill="sentinel")
    out.view.view(torch.int16).fill_(SENT)
    out.before = out.parent.view(torch.int16).clone()
    ws = Workspace(lib.gf_lora_grad_workspace_bytes(65, 72, 64))
    base = dict(Y=Y.view.data_ptr(), ldy=80, T=Tm.view.data_ptr(), ldt=72, out=out.view.data_ptr(), ldo=72, M=65, C=72, rp=64, scale=1.0, tr=0,
                ws=ws.view.data_ptr())
    bad = [
        (dict(Y=None), "null pointer"), (dict(T=None), "null pointer"), (dict(out=None), "null pointer"),
        (dict(ws=None), "null workspace"),
        (dict(M=-1), "bad shape"), (dict(C=0), "bad shape"),
        (dict(rp=0), "rank_pad=0 must be a multiple of 32 in 32..256"), (dict(rp=48), "rank_pad=48 must be a multiple of 32"),
        (dict(rp=288, ldt=288, ldo=288), "rank_pad=288 must be a multiple of 32 in 32..256"),
        (dict(C=68), "C=68 must be a multiple of 8"),
        (dict(tr=2), "transposed=2 must be 0 or 1"),
        (dict(ldy=76), "leading dimensions must be multiples of 8 and cover the row"), (dict(ldy=64), "cover the row"),
        (dict(ldt=56), "cover the row"), (dict(ldo=56), "cover the row"), (dict(tr=1, ldo=64), "cover the row"),
        (dict(Y=base["Y"] + 2), "16-byte alignment required"), (dict(T=base["T"] + 8), "16-byte alignment required"),
        (dict(out=base["out"] + 4), "16-byte alignment required"), (dict(ws=base["ws"] + 4), "16-byte alignment required"),
        (dict(M=1 << 30), "M/C too large"),
        (dict(scale=float("nan")), "scale must be finite"), (dict(scale=float("inf")), "scale must be finite"),
    ]
    for change, msg in bad:
        a = dict(base, **change)
        rc = _grad(lib, a["Y"], a["ldy"], a["T"], a["ldt"], a["out"], a["ldo"], a["M"], a["C"], a["rp"], a["scale"], a["tr"], a["ws"])
        assert rc == GF_ERR_INVALID_ARG and msg in _err(lib), (change, rc, _err(lib))
    torch.cuda.synchronize()
    assert out.untouched() and ws.guards_intact()
    assert bool(torch.isnan(ws.view.view(torch.float32)).all()), "a refusal wrote into the workspace"


def test_the_wrapper_takes_strided_views_and_refuses_by_name(ops):
    from goal_force_amd._lib import GoalForceError
    M, C, rp, r = 130, 72, 64, 33
    d = T.grad_inputs("gauss", M, C, rp, r, 0.7)
    parent = torch.full((2, M, C + 8), float("nan"), dtype=BF, device="cuda")
    y = parent[1, :, :C]
    y.copy_(d["Y"].cuda())
    t = d["T"].cuda()
    ref = T.grad_ref(d)
    got = ops.lora_grad(y, t, 0.7)
    G.assert_pinned(got.cpu(), ref, M, "ops.lora_grad on a strided view")
    # leading dimensions collapse; out= is written in place; the transposed form is the same values
    out = torch.empty((rp, C), dtype=BF, device="cuda")
    assert ops.lora_grad(d["Y"].cuda().view(2, M // 2, C), t.view(2, M // 2, rp), 0.7, transposed=True, out=out) is out
    assert torch.equal(_bits(out.cpu()), _bits(got.t().contiguous().cpu()))
    assert torch.equal(_bits(ops.lora_grad(y, t, 0.7).cpu()), _bits(got.cpu()))
    yc = d["Y"].cuda()
    for args, kw, msg in [((yc, t[:-1], 1.0), {}, r"lora_grad\.t: expected \[130, 64\] like the first operand"),
                          ((yc, t[:, :48], 1.0), {}, "last dim must be contiguous|cannot view|padded rank 48"),
                          ((yc, t[:, :32].contiguous()[:, :16], 1.0), {}, r"padded rank 16: expected a multiple of 32 in 32\.\.256"),
                          ((yc[:, :68].contiguous(), t, 1.0), {}, r"68 columns: expected a multiple of 8"),
                          ((yc.float(), t, 1.0), {}, "expected dtype"), ((yc, d["T"], 1.0), {}, "must be on the GPU"),
                          ((yc, t, float("nan")), {}, "scale must be finite"),
                          ((yc, t, 1.0), dict(out=out), r"lora_grad\.out: expected \[72, 64\]")]:
        with pytest.raises(GoalForceError, match=msg):
            ops.lora_grad(*args, **kw)


def test_figures():
    print(f"PIN lora_grad gauss: {FIG['n']} cases, worst differing share {FIG['share']:.2e} (cap 2^-10), worst ratio of (b) {FIG['worst']:.3f}")
