"""The inference forward per token row on the device, on every dispatch route: DiTBlock.forward and model_fn_wan_video against fp64
(oracle.wan_oracle) through the row statistic of tests/inference_refs.py, with the route each case names ASSERTED through counting wrappers
(a silent fall-back fails the case), and the exact relations between the forward's own call forms (out=, context_kv=, pad_n=,
self_attn_memo=, vt_from_gemm, context_cache=) bit for bit, inside NaN-filled parents.  Every threshold comes from the helper, where it is
measured on two CPU restatements against fp64 (tests/test_inference_refs_cpu.py) — none was read off the device.  `pytest -s` prints every
ratio (lines `FWD`)."""
import contextlib
import functools
import types

import pytest
import torch

import attention_fwd_refs as AF
import inference_refs as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
BLOCK = {c["name"]: c for c in R.block_cases()}
MODEL = {c["name"]: c for c in R.model_cases()}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from goal_force_amd import ops as _ops
    return _ops


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@contextlib.contextmanager
def counting(ops):
    """Wrappers around the entry points whose calls tell the route: every call is logged as (name, key rows, multiplicity, V^T given, n_pad)."""
    log = []
    real = ops.cross_probs, ops.flash_attn, ops.linear_vt32

    def cross_probs(q, k, num_heads, n_pad, last_key_mult=1, **kw):
        log.append(("cross_probs", k.shape[0], last_key_mult, False, n_pad))
        return real[0](q, k, num_heads, n_pad, last_key_mult=last_key_mult, **kw)

    def flash_attn(q, k, v, num_heads, out=None, scale=None, vt=None, last_key_mult=1, finished_q=False):
        log.append(("flash_attn", k.shape[0], last_key_mult, vt is not None, None))
        return real[1](q, k, v, num_heads, out=out, scale=scale, vt=vt, last_key_mult=last_key_mult, finished_q=finished_q)

    def linear_vt32(x, weight, bias):
        log.append(("linear_vt32", x.shape[0], 1, True, None))
        return real[2](x, weight, bias)

    ops.cross_probs, ops.flash_attn, ops.linear_vt32 = cross_probs, flash_attn, linear_vt32
    try:
        yield log
    finally:
        ops.cross_probs, ops.flash_attn, ops.linear_vt32 = real


def assert_route(log, what, tokens, L, n, cross, self_attn, blocks=1):
    """The calls of `blocks` block forwards are exactly those of the named routes.  (V^T by gf_transpose_v32 is what ops.flash_attn does
    itself when kernel 3's key count arrives without a V^T: a long call with `v`, and no linear_vt32.)"""
    kind, vt = self_attn
    want = [("flash_attn", tokens, 1, vt == "linear_vt32", None)] * blocks
    if vt == "linear_vt32":
        want += [("linear_vt32", tokens, 1, True, None)] * blocks
    assert (kind == "k3fm") == (tokens >= R.VT_MIN_KV)
    if cross == "whole":
        want += [("flash_attn", L, 1, False, None)] * blocks
    elif cross == "mult":
        want += [("flash_attn", n + 1, L - n, False, None)] * blocks
    else:
        want += [("cross_probs", n + 1, L - n, False, R.fold_pad(n + 1))] * blocks
    assert sorted(log, key=repr) == sorted(want, key=repr), f"{what}: expected the route {cross} / {self_attn}, the calls were {log}"


def _embed(t, fill=float("nan")):
    """t's values as a view inside a NaN parent: rows behind it, columns on either side (attention_fwd_refs.embed)."""
    return AF.embed(t.cuda(), 3, 8, 16, fill)


def _block_module(cfg, sd):
    from goal_force_amd.dit import DiTBlock, RopeTable, precompute_freqs_cis_3d
    blk = DiTBlock(False, cfg["dim"], cfg["num_heads"], cfg["ffn_dim"], cfg["eps"])
    blk.load_state_dict(sd, strict=True)
    return blk.to(BF).cuda(), lambda grid: RopeTable.from_grid(precompute_freqs_cis_3d(cfg["dim"] // cfg["num_heads"]), *grid, "cuda")


@functools.lru_cache(maxsize=None)
def _block_refs(name):
    """(fp64 reference, restatement of order 0) of a block case: computed once on the host and left unchanged."""
    return R.block_ref(BLOCK[name]), R.case_fwd(BLOCK[name], 0)


# ---------------------------------------------------------------------------------------------------------------------
# a. the block on every route
@pytest.mark.parametrize("name", list(BLOCK))
def test_block_every_row_on_its_route(ops, name):
    case = BLOCK[name]
    cfg, sd, x, t_mod = R.block_inputs(case["cfg"], case["grid"], case["seed"])
    ctx = R.case_ctx(case)
    ref, c0 = _block_refs(name)
    blk, rope = _block_module(cfg, sd)
    xg, cg = _embed(x)[None], _embed(ctx)[None]
    memo = {}
    with ops.options(attn_q_prescale=case["prescale"], **case["opts"]), counting(ops) as log:
        out = blk(xg, cg, t_mod.cuda(), rope(case["grid"]), self_attn_memo=memo)
    tokens = x.shape[0]
    assert_route(log, name, tokens, case["L"], R.run_start(ctx), case["cross"], case["self_attn"])
    assert out.shape == (1, tokens, cfg["dim"]) and torch.equal(xg[0].cpu(), x), "the block changed its input"
    got = types.SimpleNamespace(out=out[0].cpu(), x1=memo["x"].cpu())
    R.assert_rows(R.block_stats(got, c0, ref), f"block {name}")


# ---------------------------------------------------------------------------------------------------------------------
# b. the block's call forms, bit for bit
EXACT_CASES = ("tiny-72-norun7", "tiny-72-p30", "tiny-72-p46", "h4-130-p62", "h4-2079-p40-plainq")


@pytest.mark.parametrize("name", EXACT_CASES)
def test_block_call_forms_are_bit_identical(ops, name):
    case = BLOCK[name]
    cfg, sd, x, t_mod = R.block_inputs(case["cfg"], case["grid"], case["seed"])
    ctx = R.case_ctx(case)
    n = R.run_start(ctx)
    blk, rope_of = _block_module(cfg, sd)
    rope, tg = rope_of(case["grid"]), t_mod.cuda()
    xg, cg = _embed(x)[None], _embed(ctx)[None]
    ca = blk.cross_attn
    with ops.options(attn_q_prescale=case["prescale"]):
        base = blk(xg, cg, tg, rope)
        # out= : a view inside a NaN parent, whose surroundings stay NaN
        parent = torch.full((x.shape[0] + 5, x.shape[1] + 24), float("nan"), dtype=BF, device="cuda")
        dst = parent[2:2 + x.shape[0], 8:8 + x.shape[1]]
        ret = blk(xg, cg, tg, rope, out=dst)
        assert ret.data_ptr() == dst.data_ptr() and torch.equal(ret[0], base[0]), "out= differs from the block without it"
        mask = torch.ones_like(parent, dtype=torch.bool)
        mask[2:2 + x.shape[0], 8:8 + x.shape[1]] = False
        assert bool(torch.isnan(parent[mask]).all()), "out=: something around the destination was written"
        # context_kv handed in: (k, v, m), and with the folded table
        kv = ca.context_kv(cg[0])
        assert kv[2] == (case["L"] - n if case["cross"] != "whole" else 1) and kv[0].shape[0] == (n + 1 if case["cross"] != "whole" else case["L"])
        assert ca.fold_ok(kv) == (case["cross"] == "folded")
        with counting(ops) as log:
            assert torch.equal(blk(xg, cg, tg, rope, context_kv=kv), base), "context_kv=(k, v, m) differs"
        assert_route(log, name + " context_kv", x.shape[0], case["L"], n, case["cross"], case["self_attn"])
        if case["cross"] == "folded":
            u = ca.fold_table(kv)
            assert u.shape == (cfg["dim"], cfg["num_heads"] * R.fold_pad(n + 1))
            assert torch.equal(blk(xg, cg, tg, rope, context_kv=kv + (u,)), base), "context_kv=(k, v, m, U) differs"
        # pad_n handed in equals pad_n detected
        with counting(ops) as log:
            assert torch.equal(blk(xg, cg, tg, rope, pad_n=n), base), "pad_n handed in differs from pad_n detected"
        assert_route(log, name + " pad_n", x.shape[0], case["L"], n, case["cross"], case["self_attn"])
        # the memo: the first call stores x1 and equals the call without it; the second takes it
        memo = {}
        assert torch.equal(blk(xg, cg, tg, rope, self_attn_memo=memo), base) and set(memo) == {"x", "ev"}
        x1 = memo["x"].clone()
        with counting(ops) as log:
            assert torch.equal(blk(xg, cg, tg, rope, self_attn_memo=memo), base) and not memo, "the memoised first half differs"
        assert ("flash_attn", x.shape[0], 1, case["self_attn"][1] == "linear_vt32", None) not in log, "the memo did not save the self-attention"
        memo = {"x": x1}
        assert torch.equal(blk(xg, cg, tg, rope, self_attn_memo=memo, out=dst)[0], base[0])
        if case["self_attn"][0] == "k3fm":
            with ops.options(vt_from_gemm=False), counting(ops) as log:
                assert torch.equal(blk(xg, cg, tg, rope), base), "vt_from_gemm off differs from on"
            assert_route(log, name + " vt_from_gemm off", x.shape[0], case["L"], n, case["cross"], ("k3fm", "transpose_v32"))
    assert torch.equal(xg[0].cpu(), x) and torch.equal(cg[0].cpu(), ctx), "the block changed an input"


# ---------------------------------------------------------------------------------------------------------------------
# c. the model
def _modules(name):
    from goal_force_amd.controlnet import ControlNet
    from goal_force_amd.dit import WanModel
    cfg, dit_sd, cn_sd, inp = R.model_inputs(name)
    dit = WanModel(has_image_input=False, require_clip_embedding=False, **cfg)
    dit.load_state_dict(dit_sd, strict=True)
    cn = None
    if cn_sd is not None:
        cn = ControlNet(MODEL[name]["n_cn"], dim=cfg["dim"], num_heads=cfg["num_heads"], ffn_dim=cfg["ffn_dim"])
        cn.load_state_dict(cn_sd, strict=True)
        cn = cn.to(BF).cuda()
    return cfg, dit.to(BF).cuda(), cn, inp


@functools.lru_cache(maxsize=None)
def _model_refs(name):
    return R.model_ref(name), R.model_fwd(name, 0)


@pytest.mark.parametrize("name", list(MODEL))
def test_model_every_row_and_the_context_cache(ops, name):
    from goal_force_amd.model_fn import ContextCache, model_fn_wan_video
    case = MODEL[name]
    cfg, dit, cn, inp = _modules(name)
    ref, c0 = _model_refs(name)
    f, h, w = case["latent"][2], case["latent"][3] // 2, case["latent"][4] // 2
    tokens, n_cn, layers = f * h * w, case["n_cn"], cfg["num_layers"]
    n = R.CTX_LEN - 1 if case["p"] is None else case["p"]
    kw = dict(latents=inp["latents"].cuda(), timestep=inp["timestep"].cuda(), context=_embed(inp["context"][0])[None], y=inp["y"].cuda())
    if cn is not None:
        kw.update(controlnet=cn, control_signal_video_latents=inp["control"].cuda())
    taps = []
    hooks = [blk.register_forward_hook(lambda mod, args, out: taps.append(out.detach().clone().reshape(tokens, -1).cpu())) for blk in dit.blocks]
    try:
        with counting(ops) as log:
            out = model_fn_wan_video(dit, **kw)
    finally:
        for hk in hooks:
            hk.remove()
    assert_route(log, name, tokens, R.CTX_LEN, n, case["cross"], case["self_attn"], blocks=layers + n_cn)
    assert out.shape == tuple(case["latent"]) and len(taps) == layers
    got = types.SimpleNamespace(tok=R.tokens_of(out[0].cpu(), (f, h, w)), taps=taps)
    R.assert_rows(R.model_stats(got, c0, ref), name)
    # the context cache: a fresh one and the same one again give the bits of the forward without it, and hold exactly these entries
    cache = ContextCache()
    with counting(ops) as log:
        first = model_fn_wan_video(dit, context_cache=cache, **kw)
    assert_route(log, name + " fresh cache", tokens, R.CTX_LEN, n, case["cross"], case["self_attn"], blocks=layers + n_cn)
    assert torch.equal(first, out), "a fresh context_cache differs from none"
    held = (cache.ctx.data_ptr(), {k: v[0].data_ptr() for k, v in cache.dit_kv.items()})
    assert torch.equal(model_fn_wan_video(dit, context_cache=cache, **kw), out), "the filled context_cache differs from none"
    assert held == (cache.ctx.data_ptr(), {k: v[0].data_ptr() for k, v in cache.dit_kv.items()}), "the second call rebuilt the memo"
    folded = case["cross"] == "folded"
    assert sorted(cache.dit_kv) == list(range(layers)) and sorted(cache.cn_kv) == list(range(n_cn))
    assert sorted(cache.dit_u) == (list(range(layers)) if folded else []) and sorted(cache.cn_u) == (list(range(n_cn)) if folded else [])
    assert cache.pad_n == n, (cache.pad_n, n)
    keys, m = (R.CTX_LEN, 1) if case["cross"] == "whole" else (n + 1, R.CTX_LEN - n)
    for kv in list(cache.dit_kv.values()) + list(cache.cn_kv.values()):
        assert kv[0].shape[0] == keys and kv[1].shape[0] == keys and kv[2] == m
    assert torch.equal(kw["context"][0].cpu(), inp["context"][0]), "the model changed its context"
