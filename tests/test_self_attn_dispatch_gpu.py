"""The self-attention dispatch (dit.SelfAttention.attend, dit.DiTBlock.forward, training.DiTBlockFn's refusals) pinned as a TRACE:
which ops wrappers every configuration calls, in which order, with which operands (shape, dtype, and WHICH tensor: a model input or
an earlier call's result) and scalars, the SHA-256 of what comes back, and for a refusal its full text and that no wrapper was
reached before it.  tests/golden/self_attn_dispatch.json was recorded by this module's own `__main__` on the commit BEFORE the
dispatch was cut into named steps (`python tests/test_self_attn_dispatch_gpu.py --write tests/golden/self_attn_dispatch.json`, on
an MI355X); the tests assert that the code reproduces it exactly.  The wrappers are recorded with their arguments bound to the
wrapper's signature, defaults filled in, so `f(q, k, v, n, scale=s)` and `f(q, k, v, n, vt=None, scale=s)` — the same launch — are the
same entry.  Every weight and input has a CPU generator of its own, seeded from its name: no case depends on another.
The `fp4` cases (enable_fp4 on the FFN and / or the o projections, fused and unfused, the memo half, a weight edited under a
stale copy, the refusals) were recorded the same way on the commit BEFORE a layer's precision got one record in dit.py; each
switches fp4 on before the recorder is installed and off again, with every copy current, when it is done."""
import hashlib
import inspect
import itertools
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
BF, DEVICE = torch.bfloat16, "cuda"
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "self_attn_dispatch.json")
# dim 512 = 4 heads of 128: v.weight.shape[0] >= 512, N % 128 == 0 and K % 128 == 0 (the V^T projections), M >= 512 (the 4-wave GEMM)
DIM, HEADS, FFN = 512, 4, 1024
# long: 2304 tokens >= ops.VT_MIN_KV (kernel 3, the V^T operand, the maps); short: 72 tokens (kernel 2 on plain V)
GRIDS = {"long": (6, 16, 24), "short": (3, 4, 6)}
WRAPPERS = ("gemm", "gemm_fp8", "quant_fp8_rowscale", "layernorm_modulate", "layernorm_modulate_fp8", "rmsnorm_rope", "linear_vt32",
            "linear_vt32_fp8", "flash_attn", "flash_attn_lse", "flash_attn_sparse", "sage_attn", "cast_fp8",
            "gemm_mxfp4", "gemm_mxfp4_q4", "quant_mxfp4", "layernorm_modulate_mxfp4",
            "modulation", "cross_probs", "cross_fold_table")        # (the last three: DiTBlock.forward's other producers, for the identities)
_DTYPES = {torch.bfloat16: "bf16", torch.float32: "f32", torch.uint8: "u8", torch.int8: "i8", torch.int32: "i32",
           getattr(torch, "float8_e4m3fn", None): "e4m3"}


def _seeded(name, shape, std=1.0, mean=0.0):
    g = torch.Generator().manual_seed(int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little"))
    return torch.randn(tuple(shape), generator=g) * std + mean


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


class Recorder:
    """Wraps callables (monkeypatch.setattr) so that every call appends an entry and calls through.  A tensor is named after the
    model input it is or the entry whose result it is (`#i`, `#i.j` inside a tuple; the first name a buffer got stays), found by
    object, by data_ptr, or as `name+byte offset` inside a named tensor's storage; named tensors are held so no address is reused.
    What linear_vt32 / linear_vt32_fp8 return is the V^T WORKSPACE of the stream, as large as the largest call the process has
    made so far: its size says which tests ran before, so it is recorded as `[workspace]`."""

    def __init__(self, mp):
        self.mp, self.entries, self.by_id, self.by_ptr, self.by_storage, self.held, self.workspaces = mp, [], {}, {}, {}, [], set()

    def name(self, obj, label):
        if obj is None or isinstance(obj, (str, int, float)):
            return
        if isinstance(obj, (tuple, list)):
            for j, o in enumerate(obj):
                self.name(o, f"{label}.{j}")
            return
        self.held.append(obj)
        self.by_id.setdefault(id(obj), label)
        if torch.is_tensor(obj):
            self.by_ptr.setdefault(obj.data_ptr(), label)
            self.by_storage.setdefault(obj.untyped_storage().data_ptr(), label)

    def label(self, t):
        if id(t) in self.by_id:
            return self.by_id[id(t)]
        if torch.is_tensor(t):
            if t.data_ptr() in self.by_ptr:
                return self.by_ptr[t.data_ptr()]
            base = t.untyped_storage().data_ptr()
            if base in self.by_storage:
                return f"{self.by_storage[base]}+{t.data_ptr() - base}"
        return "?"

    def describe(self, v):
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        if isinstance(v, (tuple, list)):
            return [self.describe(o) for o in v]
        if torch.is_tensor(v):
            strides = "" if v.is_contiguous() else f"s{list(v.stride())}"
            shape = "[workspace]" if v.data_ptr() in self.workspaces else list(v.shape)
            return f"{_DTYPES.get(v.dtype, str(v.dtype))}{shape}{strides}:{self.label(v)}"
        if type(v).__name__ == "BlockMap":
            return f"BlockMap[{v.n_maps},{v.n_qblocks},{v.n_tiles}]@{v.device.type}:{self.label(v)}"
        return type(v).__name__

    def wrap(self, owner, attr, op):
        fn = getattr(owner, attr)
        sig = inspect.signature(fn)

        def wrapped(*a, **k):
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            i = len(self.entries)
            self.entries.append({"op": op, "args": {n: self.describe(v) for n, v in bound.arguments.items()}})
            out = fn(*a, **k)
            self.name(out, f"#{i}")
            if op.startswith("linear_vt32"):
                self.workspaces.add(out.data_ptr())
            return out
        self.mp.setattr(owner, attr, wrapped)


class StubSP:
    """A duck-typed one-rank sequence_parallel.SequenceParallel: no process group, no collective.  The exchanges hand the tensor
    back; the attention is the backend's, on the wrappers the recorder holds."""
    size, rank = 1, 0

    def __init__(self, ops):
        self.ops = ops

    def _attn(self, backend):
        return self.ops.sage_attn if backend == "sage" else self.ops.flash_attn

    def heads_start(self, t, num_heads=None):
        return ("work", t)

    def attention_started(self, hq, hk, hv, num_heads, out_shape, scale=None, backend="flash"):
        return self._attn(backend)(hq[1], hk[1], hv[1], num_heads, scale=scale)

    def attention(self, q, k, v, num_heads, scale=None, backend="flash"):
        return self._attn(backend)(q, k, v, num_heads, scale=scale)


# ---- the cases.  attend: the full product — every term either runs or is refused by name before the first wrapper (sage x keep, and
# a sparse block with sage / keep / sp / the short grid), so nothing is skipped as unreachable.
LINEARS, BACKENDS, SPARSITY = ("bf16", "fp8"), ("flash", "sage"), ("none", "window", "masscover", "window_dense")
SPS, KEEPS, OPTIONS = ("nosp", "sp"), ("nokeep", "keep", "wide"), ("attn_q_prescale", "vt_from_gemm", "attn_k3")
CASES = ["attend-" + "-".join(c) for c in itertools.product(LINEARS, BACKENDS, SPARSITY, SPS, KEEPS, GRIDS)]
CASES += [f"attend-option-{o}" for o in OPTIONS]                                   # each switched OFF on the plain bf16 long case
CASES += [f"blockfn-{kind}-{level}" for kind in ("fp8", "sage", "sparse") for level in ("none", "attn")]
CASES += [f"block-{lin}-{memo}" for lin in LINEARS for memo in ("nomemo", "memo")]  # DiTBlock.forward, first and second call
# enable_fp4 on top of either block: one forward per layer set and FFN route; the memo half; a weight edited under its copy (two
# forwards: the first refreshes the copy, once; the second finds it current); what is refused by name before the first wrapper
CASES += [f"block-{lin}-fp4{layers}-{route}" for lin in LINEARS for layers in ("ffn", "o", "ffn+o") for route in ("fused", "unfused")]
CASES += ["block-fp8-fp4ffn+o-fused-memo", "block-fp8-stale", "block-bf16-fp4ffn-stale"]
CASES += ["linear-fp8input-fp4o", "blockfn-fp4-none", "blockfn-fp4-attn", "enablefp4-q", "enablefp4-k128"]


class Env:
    """The two blocks (bf16 linears, enable_fp8) with the same seeded weights, and the seeded inputs, on the GPU."""

    def __init__(self):
        from goal_force_amd import dit
        self.blocks = {}
        for lin in LINEARS:
            blk = dit.DiTBlock(False, DIM, HEADS, FFN)
            for n, p in blk.named_parameters():
                if n.endswith("modulation"):
                    p.data = _seeded(n, p.shape, DIM ** -0.5)
                elif n.endswith(".bias"):
                    p.data = _seeded(n, p.shape, 0.02)
                elif p.dim() == 2:
                    p.data = _seeded(n, p.shape, p.shape[1] ** -0.5)
                else:
                    p.data = _seeded(n, p.shape, 0.1, 1.0)              # norm weights
            blk = blk.to(BF).to(DEVICE).requires_grad_(False)
            self.blocks[lin] = dit.enable_fp8(blk) if lin == "fp8" else blk
        freqs3 = dit.precompute_freqs_cis_3d(DIM // HEADS)
        self.rope = {g: dit.RopeTable.from_grid(freqs3, *grid, DEVICE) for g, grid in GRIDS.items()}
        self.x = {g: _seeded(f"x-{g}", (r.tokens, DIM)).to(BF).to(DEVICE) for g, r in self.rope.items()}
        ctx = _seeded("context", (20, DIM))
        ctx[12:] = ctx[12]                                              # a padded tail of 8 identical rows: the folded cross-attention
        self.ctx = ctx.to(BF).to(DEVICE)
        self.t_mod = _seeded("t_mod", (1, 6, DIM), 0.1).to(BF).to(DEVICE)

    def name_inputs(self, rec, blk, g):
        from goal_force_amd import dit
        rope = self.rope[g]
        for label, t in (("x", self.x[g]), ("context", self.ctx), ("t_mod", self.t_mod), ("rope.cos", rope.cos), ("rope.sin", rope.sin),
                         *zip(("rope.cos*c", "rope.sin*c"), rope.scaled(dit.Q_PRESCALE(DIM // HEADS)))):
            rec.name(t, label)
        for n, p in blk.named_parameters():
            rec.name(p, n)
        for n, m in blk.named_modules():
            for kind in ("w8", "w4"):                                   # (an fp4 copy is (codes, scales): `<layer>.w4.0` / `.w4.1`)
                if getattr(m, "_gf_" + kind, None) is not None:
                    rec.name(getattr(m, "_gf_" + kind), f"{n}.{kind}")


def _pattern(kind):
    from goal_force_amd.sparse_attention import FrameWindow, MassCover
    return {"none": None, "window": FrameWindow(1, 1), "window_dense": FrameWindow(1, 1),
            "masscover": MassCover(0.9, always=FrameWindow(1, 1))}[kind]


def _attend(env, rec, lin, backend, sparsity, sp, keep, g):
    from goal_force_amd import dit, ops
    blk = env.blocks[lin]
    pattern = _pattern(sparsity)
    if pattern is not None and hasattr(pattern, "from_qk"):
        rec.wrap(pattern, "from_qk", "pattern.from_qk")
    stub = None
    if sp == "sp":
        stub = StubSP(ops)
        for m in ("heads_start", "attention_started", "attention"):
            rec.wrap(stub, m, "sp." + m)
    kept = {"nokeep": None, "keep": {}, "wide": {"wide": True}}[keep]
    dit.enable_sage_attention(blk, backend == "sage")
    dit.enable_sparse_attention(blk, pattern)
    try:
        out = blk.self_attn.attend(env.x[g], env.rope[g], stub, kept, dense=sparsity == "window_dense")
    finally:
        dit.enable_sage_attention(blk, False)
        dit.enable_sparse_attention(blk, None)
    res = {"out": rec.describe(out), "sha256": _sha(out)}
    if kept is not None:
        res["keep"] = {n: (rec.describe(v), _sha(v)) if torch.is_tensor(v) else v for n, v in sorted(kept.items())}
    return res


def _blockfn(env, rec, kind, level):
    from goal_force_amd import dit, training
    blk = env.blocks["fp8" if kind == "fp8" else "bf16"]
    dit.enable_sage_attention(blk, kind == "sage")
    dit.enable_sparse_attention(blk, _pattern("window") if kind == "sparse" else None)
    old = training.set_keep_level(level)
    try:
        out = training.DiTBlockFn.apply(blk, env.rope["long"], env.x["long"], env.ctx, env.t_mod, *training._block_params(blk))
    finally:
        training.set_keep_level(old)
        dit.enable_sage_attention(blk, False)
        dit.enable_sparse_attention(blk, None)
    return {"out": rec.describe(out), "sha256": _sha(out)}          # (not reached: every one of these is refused)


def _block(env, rec, lin, *flags, calls=("first", "second")):
    """DiTBlock.forward once per name in `calls`.  flags: memo | nomemo; unfused (ops.options(fp4_fused=False)); stale (ffn[0]'s
    weight doubled in place under its current copy before the first call: run_case halves it again)."""
    from goal_force_amd import ops
    blk = env.blocks[lin]
    memo = {} if "memo" in flags else None
    res = {}
    if "stale" in flags:
        blk.ffn[0].weight.mul_(2.0)
    with ops.options(fp4_fused="unfused" not in flags):
        for call in calls:
            out = blk(env.x["long"][None], env.ctx[None], env.t_mod, env.rope["long"], self_attn_memo=memo)
            res[call] = {"out": rec.describe(out), "sha256": _sha(out), "calls_so_far": len(rec.entries),
                         "memo": None if memo is None else sorted(memo)}
    return res


def _fp4_layers(kind, rest):
    """The enable_fp4 layer names a case switches on before its recording starts (() for a case without fp4)."""
    if kind == "block":
        return tuple(n for f in rest if f.startswith("fp4") for n in f[3:].split("+"))
    return {("blockfn", "fp4"): ("ffn", "o"), ("linear", "fp8input"): ("o",)}.get((kind, rest[0]), ())


def run_case(env, case, mp):
    """One case -> its record: {"calls": [entries], ...result} or {"refused": text, "calls_before": n}."""
    from goal_force_amd import ops
    from goal_force_amd._lib import GoalForceError
    from goal_force_amd import dit
    kind, *rest = case.split("-")
    g = rest[-1] if kind == "attend" and rest[0] != "option" else "long"
    lin = "fp8" if rest[0] == "fp8" else "bf16"
    blk, fp4 = env.blocks[lin], _fp4_layers(kind, rest)
    if fp4:                                         # before the recorder: the case is what runs on the switched block
        dit.enable_fp4(blk, layers=fp4)
    x8 = dit.QuantizedInput(env.x["short"]) if kind == "linear" else None
    rec = Recorder(mp)
    for w in WRAPPERS:
        rec.wrap(ops, w, w)
    env.name_inputs(rec, blk, g)
    try:
        with torch.no_grad():
            if kind == "attend" and rest[0] == "option":
                with ops.options(**{rest[1]: False}):
                    res = _attend(env, rec, "bf16", "flash", "none", "nosp", "nokeep", "long")
            elif kind == "attend":
                res = _attend(env, rec, *rest)
            elif kind == "blockfn":
                res = _blockfn(env, rec, *rest)
            elif kind == "linear":
                res = {"out": rec.describe(dit.linear(x8, blk.self_attn.o))}        # (not reached: refused)
            elif kind == "enablefp4":
                res = {"out": rec.describe(dit.enable_fp4(dit.DiTBlock(False, 128, 1, 128) if rest[0] == "k128" else blk,
                                                          layers=("ffn", "o") if rest[0] == "k128" else (rest[0],)))}
            else:
                two = any(f in ("memo", "nomemo", "stale") for f in rest)
                res = _block(env, rec, *rest, calls=("first", "second") if two else ("first",))
        record = json.loads(json.dumps({"calls": rec.entries, **res}))
    except GoalForceError as e:
        record = {"refused": str(e), "calls_before": len(rec.entries)}
    finally:
        mp.undo()                                   # the recording is over: what follows leaves the block as the case found it
        if fp4:
            dit.enable_fp4(blk, False, layers=fp4)
        if "stale" in rest:
            with torch.no_grad():
                blk.ffn[0].weight.mul_(0.5)         # exact: the bf16 master is the seeded one again
            dit.fp8_weight(blk.ffn[0])              # and the copy current (fp4's left with enable_fp4(False))
    return record


@pytest.fixture(scope="module")
def env():
    return Env()


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(recorded):
    assert sorted(recorded) == sorted(CASES)


def test_a_stale_copy_is_refreshed_once_and_only_on_the_first_call(recorded):
    for case, op in (("block-fp8-stale", "cast_fp8"), ("block-bf16-fp4ffn-stale", "quant_mxfp4")):
        calls, first = recorded[case]["calls"], recorded[case]["first"]["calls_so_far"]
        at = [i for i, c in enumerate(calls) if c["op"] == op and any(str(v).endswith(":ffn.0.weight") for v in c["args"].values())]
        assert len(at) == 1 and at[0] < first, (case, at, first)


@pytest.mark.parametrize("case", CASES)
def test_dispatch_reproduces_the_recorded_trace(env, recorded, monkeypatch, case):
    got, want = run_case(env, case, monkeypatch), recorded[case]
    if "refused" in want:
        assert want["calls_before"] == 0, "a refusal comes before the first kernel wrapper"
    if got != want and "calls" in got and "calls" in want:
        for i, (a, b) in enumerate(zip(got["calls"], want["calls"])):
            assert a == b, f"call #{i} differs"
    assert got == want


if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
    target = sys.argv[sys.argv.index("--write") + 1]
    e, records = Env(), {}
    for c in CASES:
        with pytest.MonkeyPatch.context() as mp_:
            records[c] = run_case(e, c, mp_)
    with open(target, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(c)}: {json.dumps(r)}" for c, r in records.items()) + "\n}\n")
    n_ref = sum("refused" in r for r in records.values())
    import goal_force_amd
    print(f"{goal_force_amd.__file__}: {len(records)} cases ({n_ref} refusals, {sum(len(r.get('calls', ())) for r in records.values())} wrapper calls) -> {target}")
