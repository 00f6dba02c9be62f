"""bench.py as the driver launches it (BASELINE config 3's code path): `--gpus 2` = one CFG pair, two fresh
processes with the torch.distributed.run environment, per-step noise-prediction all-gather, tiled VAE decode split over
the pair, end-of-run frame all-gather.  The GPU box has ONE device, so the two ranks share cuda:0 and rendezvous over
gloo (GF_DIST_BACKEND=gloo; RCCL wants one device per rank) — same code path, different transport.
Property checked: sharding the CFG pair over two ranks changes no bit — latents and uint8 frames of the N=2 run equal the
N=1 run's (bench.py prints their sha256 in `self_check`).  World 4 = two videos x CFG pair (BASELINE config 3's layout at half
size): every video's latents and frames — the frames as rank 0 RECEIVED them from the leads-only all-gather — equal the N=1 run
of that video."""
import json
import os
import socket
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
# the sharding tests time two layers; the extra legs of the N = 1 line (config 5, data sensitivity, pre-loop) have their own test below.
# --full: the self-check digests and the roofline entries these tests read are not part of a plain run
ARGS = ["--full", "--layers", "2", "--steps", "2", "--warmup", "0", "--no-cpu-baseline", "--config5-steps", "0", "--peaky-steps", "0", "--no-preloop", "--no-yardstick"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_RUNS = {}


def _launch(world, extra=(), args=None):
    """One bench.py run (its JSON line); identical invocations are launched ONCE per test session and shared (the N = 1 two-layer
    run is the yardstick of three tests)."""
    extra = tuple(a for a in extra)
    if extra == ("--sample-offset", "0"):
        extra = ()                                  # the default
    key = (world, extra, None if args is None else tuple(args))
    if key not in _RUNS:
        _RUNS[key] = _launch_now(world, extra, ARGS if args is None else list(args))
    return _RUNS[key]


def _launch_now(world, extra, args):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), GF_DIST_BACKEND="gloo")
        if world == 1:
            for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
                env.pop(k)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world)] + args + list(extra),
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=1500) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, so[-2000:] + se[-4000:]
    lines = [l for l in outs[0][0].splitlines() if l.startswith("{")]
    assert len(lines) == 1, outs[0][0][-2000:]
    assert not any(l.startswith("{") for so, _ in outs[1:] for l in so.splitlines()), "only rank 0 prints the JSON line"
    return json.loads(lines[0])


def test_bench_two_ranks_bit_identical_to_one():
    one = _launch(1)
    two = _launch(2)
    for j, n in ((one, 1), (two, 2)):
        assert j["n_gpus"] == n and j["steps"] == 2 and j["unit"] == "frames/s" and j["value"] > 0
        assert j["self_check"]["latents_finite"] and j["self_check"]["frames_finite"]
        assert j["roofline"]["achieved"] > 0 and j["roofline_gemm"]
    assert two["distributed"] == {**two["distributed"], "world": 2, "backend": "gloo", "rccl_ranks": 0}
    assert one["distributed"]["world"] == 1 and one["frame_allgather_s"] == 0.0
    assert two["frame_allgather_s"] > 0 and two["samples_gathered"] == 1
    # the N > 1 pre-flight ran every collective of the path once before the timed region and reports the layout
    pf = two["preflight"]
    assert set(pf["steps"]) == {"noise_pred_allgather_pair", "vae_tile_broadcast_pair", "frames_allgather_leads"} and pf["rccl_ranks"] == 0
    assert pf["steps"]["noise_pred_allgather_pair"]["bytes"] == 2 * 16 * 21 * 60 * 104 * 2 and pf["steps"]["frames_allgather_leads"]["bytes"] == 81 * 480 * 832 * 3
    assert [(r["rank"], r["sample"], r["branch"]) for r in pf["ranks"]] == [(0, 0, 0), (1, 0, 1)] and pf["min_hbm_free_gb"] > 1
    assert "preflight" not in one
    assert two["self_check"]["latents"]["sha256"] == one["self_check"]["latents"]["sha256"]
    assert two["self_check"]["frames_uint8"]["sha256"] == one["self_check"]["frames_uint8"]["sha256"]
    assert "cpu_baseline" not in two


# BASELINE config 3's WORKLOAD: the production model — 40 DiT + 10 ControlNet blocks, both experts, S = 32760 — not a
# two-layer stand-in.  K = 2 puts one timed step on each side of the expert switch (step ids 12 and 37).
FULL = ["--full", "--steps", "2", "--warmup", "0", "--no-cpu-baseline", "--config5-steps", "0", "--peaky-steps", "0", "--no-preloop", "--no-yardstick"]


def test_bench_cfg_pair_at_production_size_bit_identical_to_one_gpu():
    """`bench.py --gpus 2 --steps 2 --warmup 0` at FULL size over gloo on the box's one GPU (2 ranks x 71 GB of weights): the
    pre-flight moves every collective of the path at its production byte count, the CFG pair exchanges the 4.19 MB noise prediction
    per step, the VAE tiles are split over the pair, the leads gather the frames — and latents and uint8 frames equal the N = 1 run of
    the same step ids bit for bit.  (RCCL between two devices is the one thing a one-GPU box cannot show: SCALE run)"""
    two = _launch(2, args=FULL)
    one = _launch(1, args=FULL)
    for j, n in ((one, 1), (two, 2)):
        assert j["n_gpus"] == n and j["steps"] == 2 and j["config"]["layers"] == 40 and "[12, 37]" in j["config"]["schedule"]
        assert j["denoise_step_ms_high_noise"] > j["denoise_step_ms_low_noise"] > 0
    pf = two["preflight"]
    assert {k: v["bytes"] for k, v in pf["steps"].items()} == {"noise_pred_allgather_pair": 8386560, "vae_tile_broadcast_pair": 129392640,
                                                               "frames_allgather_leads": 97044480}
    assert [(r["rank"], r["sample"], r["branch"]) for r in pf["ranks"]] == [(0, 0, 0), (1, 0, 1)]
    assert pf["min_hbm_free_gb"] > 20, "two full-size ranks on one 288 GB device leave room for the activations"
    assert two["distributed"]["world"] == 2 and two["distributed"]["backend"] == "gloo" and two["samples_gathered"] == 1
    assert two["self_check"]["latents"]["sha256"] == one["self_check"]["latents"]["sha256"]
    assert two["self_check"]["frames_uint8"]["sha256"] == one["self_check"]["frames_uint8"]["sha256"]
    # a rank of the pair runs ONE forward per step: with both ranks time-sharing one device the pair's step costs what the N = 1 step costs
    # plus the lost sharing of block 0 — a gross error in the sharding (both ranks computing both branches) would double it
    assert two["denoise_step_ms_high_noise"] < 1.5 * one["denoise_step_ms_high_noise"]
    out = os.path.join(ROOT, "gpurun_out", "r06")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "bench_n2_fullsize_in_suite.json"), "w") as f:
        json.dump({"n2": two, "n1": one}, f, indent=1)


def test_bench_four_ranks_two_videos_bit_identical_to_single_runs():
    four = _launch(4)
    assert four["n_gpus"] == 4 and four["samples_gathered"] == 2 and four["frame_allgather_s"] > 0
    assert four["distributed"]["world"] == 4 and four["distributed"]["backend"] == "gloo"
    per = four["self_check"]["per_sample"]
    assert [d["sample"] for d in per] == [0, 1]
    assert per[0]["frames_uint8_sha256"] != per[1]["frames_uint8_sha256"], "the two videos have different seeds"
    for k in (0, 1):
        one = _launch(1, ["--sample-offset", str(k)])
        (d,) = one["self_check"]["per_sample"]
        assert d["sample"] == k
        assert per[k]["latents_sha256"] == d["latents_sha256"], f"video {k}: latents of the 4-rank run differ from its N=1 run"
        assert per[k]["frames_uint8_sha256"] == d["frames_uint8_sha256"], f"video {k}: gathered frames differ from its N=1 run"


def _one_json(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def _clean_env(**kv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    env.update(GF_DIST_BACKEND="gloo", **kv)
    return env


def test_bench_self_launch_and_torchrun_agree():
    """`python bench.py --gpus 2` with NO launcher (the parent spawns its own two ranks) and the same run through
    `python -m torch.distributed.run` — the form the driver uses — print one JSON line each with identical latents / frames."""
    cmd = [os.path.join(ROOT, "bench.py"), "--gpus", "2"] + ARGS
    r = subprocess.run([sys.executable] + cmd, env=_clean_env(), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    own = _one_json(r.stdout)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(_free_port())] + cmd, env=_clean_env(), capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    tr = _one_json(r.stdout)
    for j in (own, tr):
        assert j["n_gpus"] == 2 and j["distributed"]["world"] == 2 and j["distributed"]["backend"] == "gloo"
    assert own["self_check"]["latents"]["sha256"] == tr["self_check"]["latents"]["sha256"]
    assert own["self_check"]["frames_uint8"]["sha256"] == tr["self_check"]["frames_uint8"]["sha256"]


def test_bench_self_launch_eight_ranks_and_failure_exit_code():
    """BASELINE config 3's layout (4 videos x CFG pair = 8 ranks) through bench.py itself, self-launched, one block deep over
    gloo on the one GPU of the box: four different videos gathered on rank 0.  And a rank that fails makes the parent exit
    non-zero instead of hanging the others (--sp 3 is refused by every rank)."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "8", "--layers", "1", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"]
    r = subprocess.run(cmd, env=_clean_env(), capture_output=True, text=True, timeout=2400)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    j = _one_json(r.stdout)
    assert j["n_gpus"] == 8 and j["samples_gathered"] == 4 and j["distributed"]["world"] == 8
    per = j["self_check"]["per_sample"]
    assert [d["sample"] for d in per] == [0, 1, 2, 3] and len({d["frames_uint8_sha256"] for d in per}) == 4
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--sp", "3"] + ARGS, env=_clean_env(),
                         capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and not any(l.startswith("{") for l in bad.stdout.splitlines())


def test_bench_line_is_schedule_weighted_and_carries_preloop_vae_roofline_and_data_sensitivity():
    """What SURVEY §8(d) asks of the driver-visible line, on a 2-layer model so that it runs in a minute:
    `value` is the 21 : 29 schedule-weighted figure; `preloop` = two tiled VAE encodes + two umT5-XXL forwards at full size, reported
    beside it and not inside it; `roofline_vae` = the decode's three dominant convolution launches; `data_sensitivity` = the same
    steps with the attention logits x 8; `config5` without an error."""
    j = _launch(1, args=[a for a in ARGS if a not in ("--no-preloop", "--no-yardstick")] + ["--config5-steps", "2", "--peaky-steps", "2"])   # (argparse keeps the LAST value)
    assert "error" not in j["config5"] and j["config5"]["steps"] == 2 and j["config5"]["ms_per_step"] > 0
    hi, lo, vs = j["denoise_step_ms_high_noise"], j["denoise_step_ms_low_noise"], j["vae_decode_s"]
    assert hi > lo > 0, "a high-noise step runs the ControlNet on top of the DiT"
    want = 81.0 / ((21 * hi + 29 * lo) / 1e3 + vs)
    assert abs(j["value"] - want) <= 1e-9 * want, (j["value"], want)
    assert abs(j["denoise_loop_s_50_steps"] - (21 * hi + 29 * lo) / 1e3) < 1e-9 and "21 x mean high-noise" in j["config"]["value_definition"]
    assert j["ms_per_step"] > 0 and j["frames_per_sec_unweighted"] > 0
    ds = j["data_sensitivity"]
    assert "error" not in ds and ds["steps"] == 2 and ds["denoise_step_ms_high_noise"] > 0 and ds["self_attention_avg_launch_ms"] > 0
    rv = j["roofline_vae"]
    assert len(rv) == 3 and all(0 < e["frac"] < 1 and e["bound"] == "mfma" and e["launches"] > 0 and e["algorithmic_flops_per_launch"] > 1e11
                                for e in rv)
    assert sum(e["share_of_decode_conv_time"] for e in rv) > 0.5, "the three entries are the bulk of the decode's convolution time"
    assert 0.5 * vs * 1e3 < j["vae_decode_conv_ms"] < 1.05 * vs * 1e3, "the convolutions are most of the tiled decode"
    hb = j["host_boundary"]                      # the PCIe crossings + PIL wrapping of the B1 boundary, beside `value`
    assert "error" not in hb and hb["h2d_bytes"] == 81 * 480 * 832 * 3 * 2 and hb["d2h_bytes"] == 81 * 480 * 832 * 3
    assert 0 < hb["frames_per_sec_pcie_inclusive"] < j["value"] and hb["frames_per_sec_pcie_inclusive"] > 0.7 * j["value"]
    # `gpu_eager_yardstick`: the same step through torch-ROCm's own kernels, beside the line and never inside `value`
    ys = j["gpu_eager_yardstick"]
    assert "error" not in ys, ys
    assert ys["denoise_step_ms_high_noise"] > 0 and ys["denoise_step_ms_low_noise"] >= ys["denoise_step_ms_low_noise_controlnet2_elided"] * 0.9
    assert abs(ys["denoise_loop_s_50_steps"] - (21 * ys["denoise_step_ms_high_noise"] + 29 * ys["denoise_step_ms_low_noise"]) / 1e3) < 1e-9
    assert abs(ys["speedup_denoise_loop"] - ys["denoise_loop_s_50_steps"] / j["denoise_loop_s_50_steps"]) < 1e-9
    assert ys["speedup_denoise_loop"] > 1.0, "the HIP path is faster than the eager stack on the same GPU"
    # `preloop` (on by default in the driver's command): 2 tiled VAE encodes of an 81-frame 480x832 clip + 2 umT5-XXL forwards, full size
    pl = j["preloop"]
    assert "error" not in pl, pl
    assert 0.05 < pl["vae_tiled_encode_x2_s"] < 10 and 0.005 < pl["umt5_xxl_512_tokens_x2_s"] < 10 and pl["umt5_xxl_params"] > 5e9
    assert abs(pl["total_s"] - pl["vae_tiled_encode_x2_s"] - pl["umt5_xxl_512_tokens_x2_s"]) < 1e-9


def test_bench_head_parallel_pair_bit_identical_to_one_gpu():
    """`bench.py --gpus 4 --sp 2`: one video, its CFG pair, every forward head-parallel over two ranks (Ulysses exchanges started
    as soon as each projection is ready, the head group in two halves; sequence_parallel.py) — the pre-flight runs the head
    all-to-all at production size, and latents and frames equal the one-GPU run bit for bit."""
    one = _launch(1)
    sp = _launch(4, ["--sp", "2"])
    assert sp["n_gpus"] == 4 and sp["samples_gathered"] == 1 and "head-parallel attention degree 2" in sp["config"]["parallelism"]
    assert set(sp["preflight"]["steps"]) == {"noise_pred_allgather_pair", "vae_tile_broadcast_pair", "frames_allgather_leads", "head_all_to_all_sp_group"}
    assert [(r["sample"], r["branch"], r["sp_rank"]) for r in sp["preflight"]["ranks"]] == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1)]
    assert sp["self_check"]["latents"]["sha256"] == one["self_check"]["latents"]["sha256"]
    assert sp["self_check"]["frames_uint8"]["sha256"] == one["self_check"]["frames_uint8"]["sha256"]


def test_bench_plain_line_is_lean_and_dumps_the_timed_outputs(tmp_path):
    """A plain run (no --full) times the steps and the VAE decode and prints the headline only — none of the extra legs — and
    `--dump-outputs DIR` writes what its timed path returned: the latents are bit for bit the ones the --full run of the same
    steps reports in `self_check`, and the dump stays under 64 MB."""
    import hashlib

    import numpy as np
    import torch
    one = _launch(1)
    out = tmp_path / "outputs"
    j = _launch_now(1, (), ["--layers", "2", "--steps", "2", "--warmup", "0", "--dump-outputs", str(out)])
    assert j["steps"] == 2 and j["ms_per_step"] > 0 and j["value"] > 0 and j["higher_is_better"] is True
    assert (j["metric"], j["unit"], j["dtype"]) == (one["metric"], one["unit"], one["dtype"])
    for leg in ("self_check", "roofline", "roofline_gemm", "roofline_vae", "config5", "data_sensitivity", "preloop", "host_boundary",
                "gpu_eager_yardstick", "cpu_baseline"):
        assert leg not in j, f"a plain run carries `{leg}`"
    lat, frames = np.load(out / "latents.npy"), np.load(out / "frames.npy")
    assert lat.dtype == np.float32 and lat.shape == (1, 16, 21, 60, 104)
    assert frames.dtype == np.float32 and frames.shape == (1, 3, 9, 480, 832) and np.isfinite(frames).all()
    raw = torch.from_numpy(lat).to(torch.bfloat16).view(torch.int16).numpy().tobytes()
    assert hashlib.sha256(raw).hexdigest() == one["self_check"]["latents"]["sha256"]
    assert sum(f.stat().st_size for f in out.iterdir()) <= 64e6
