"""bench.py end to end: the single-process line, and the multi-rank launch the driver uses (two ranks sharing cuda:0 through
STLT_BENCH_ONE_GPU=1 / gloo, since the test box has one GPU): one JSON line on rank 0 with the contract's fields.  A plain run prints
that line alone (and writes the last timed step's outputs with --dump-outputs); --full adds the rooflines, side legs and CPU baseline."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
PLAIN = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
         "data", "config"}
REQUIRED = PLAIN | {"roofline"}


def _last_json(stdout: str, with_legs=False):
    """The contract line is the LAST JSON line and stays under 6 KB (the driver keeps an 8-KB tail of stdout); every line before it is
    a side measurement's own object, {"leg": name, ...}."""
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert lines, stdout[-2000:]
    assert len(lines[-1]) < 6144, len(lines[-1])
    head = json.loads(lines[-1])
    legs = {}
    for l in lines[:-1]:
        j = json.loads(l)
        assert "leg" in j and "metric" not in j, l[:200]
        legs[j.pop("leg")] = j
    assert "leg" not in head
    for name, summary in head.get("legs", {}).items():  # the last line's four-number summaries are the legs' own numbers
        assert name in legs, (name, sorted(legs))
        if isinstance(summary, list):
            assert summary[0] == legs[name]["value"] and summary[1] == legs[name]["ms_per_step"], (name, summary)
    return (head, legs) if with_legs else head


def test_single_process_line():
    r = subprocess.run([sys.executable, "bench.py", "--full", "--steps", "2", "--warmup", "1", "--batch", "64"], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, STLT_BENCH_CPU_BUDGET_S="2"))
    assert r.returncode == 0, r.stderr[-2000:]
    j = _last_json(r.stdout)
    assert REQUIRED <= set(j) and j["n_gpus"] == 1 and j["value"] > 0 and j["unit"] == "clips/s" and j["scaling"] == "weak"
    assert j["config"]["per_gpu_batch"] == 64 and "workload" in j["config"]
    assert set(j["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"}
    assert j["cpu_baseline"]["value"] > 0 and j["cpu_baseline"]["kind"] == "port"
    assert j["legs"]["skip_padding"][0] > j["value"] and j["logit_max_abs_diff"] <= 1e-4
    assert j["roofline_attn_temporal"]["bound"] == "hbm" and j["roofline_attn_temporal"]["frac"] > 0


def test_plain_line_is_the_timed_steps_and_dumps_the_last_one(pkg, tmp_path):
    """A plain run: the contract line alone, priced on exactly --steps timed steps; --dump-outputs holds the logits of the last one, which
    are the oracle's for the seeded batch."""
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--batch", "64", "--dump-outputs", str(out)], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert PLAIN <= set(j) and not {"roofline", "legs", "cpu_baseline"} & set(j), sorted(j)
    assert j["steps"] == 3 and j["warmup"] == 1 and j["n_gpus"] == 1 and j["config"]["per_gpu_batch"] == 64
    assert j["unit"] == "clips/s" and j["higher_is_better"] is True and j["dtype"] == "f32" and j["metric"].startswith("clips/s STLT forward")
    assert j["ms_per_step"] > 0 and abs(j["value"] - 64 / (j["ms_per_step"] * 1e-3)) <= 1e-3 * j["value"]
    assert sorted(os.listdir(out)) == ["stlt.npy"]
    logits = np.load(out / "stlt.npy")
    c = pkg.synth.CONFIGS["cfg2"]
    assert logits.dtype == np.float32 and logits.shape == (64, c["num_classes"]) and np.isfinite(logits).all()
    from oracle import stlt_oracle as O
    model = pkg.Stlt(pkg.StltModelConfig(**pkg.synth.model_kwargs("cfg2")))
    sd = pkg.synth.make_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1234)
    batch = pkg.synth.make_batch(64, c["T"], c["N"], dataset=c["dataset"], seed=1000)
    with torch.no_grad():
        ref = O.stlt_forward(sd, {k: v[:4] for k, v in batch.items()}, c["num_attention_heads"])["stlt"].numpy()
    assert np.abs(logits[:4] - ref).max() <= 1e-4


def test_train_mode_plain_line_dumps_the_last_step(tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, "bench.py", "--mode", "train", "--steps", "2", "--warmup", "1", "--batch", "8", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert PLAIN <= set(j) and not {"roofline", "cpu_baseline", "kernel_ms_per_step"} & set(j), sorted(j)
    assert j["steps"] == 2 and "train step" in j["metric"] and j["ms_per_step"] > 0
    assert sorted(os.listdir(out)) == ["grad_norm.npy", "loss.npy", "params_sample.npy"]
    loss, gn, prm = (np.load(out / f"{n}.npy") for n in ("loss", "grad_norm", "params_sample"))
    assert loss.dtype == np.float32 and abs(float(loss[0]) - j["loss"]) <= 1e-6 * max(1.0, abs(j["loss"])) and float(gn[0]) > 0
    assert prm.dtype == np.float32 and prm.shape == (1 << 20,) and np.isfinite(prm).all()


def test_side_legs_ride_on_the_default_line():
    """train_step / cfg4 / small_batch sub-objects (BASELINE configs 3, 4 and the reference's default batch) next to `value`."""
    r = subprocess.run([sys.executable, "bench.py", "--full", "--steps", "2", "--warmup", "1", "--batch", "256", "--side-legs", "--no-cpu-baseline",
                        "--no-skip-padding"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    head, j = _last_json(r.stdout, with_legs=True)
    for key in ("dense_schedule", "train_step", "cfg4", "small_batch", "cfg2p", "ref_default", "cfg2p_b64", "ref_default_b64", "skip_padding_b64", "cfg5",
                "cfg5_train", "split_bf16"):
        assert isinstance(head["legs"][key], list) and head["legs"][key][0] > 0, (key, head["legs"].get(key))
    for key in ("train_step", "small_batch", "cfg2p_b64", "ref_default_b64", "cfg5_train"):  # [clips/s, ms, GEMM fraction, temporal-core fraction]
        assert 0 < head["legs"][key][2] < 1, (key, head["legs"][key])
    assert 0 < head["legs"]["small_batch"][3] < 1 and 0 < head["legs"]["ref_default_b64"][3] < 1
    assert j["skip_padding_b64"]["value"] > j["small_batch"]["value"]
    assert "error" not in j["cfg5_train"] and j["cfg5_train"]["value"] > 0 and j["cfg5_train"]["grad_norm"] > 0 and 0 < j["cfg5_train"]["roofline"]["frac"] < 1, j["cfg5_train"]
    assert "error" not in j["cfg5"] and j["cfg5"]["value"] > 0 and j["cfg5"]["finite"] and 0 < j["cfg5"]["roofline"]["frac"] < 1, j["cfg5"]
    for key in ("train_step", "cfg4", "small_batch"):
        assert "error" not in j[key], j[key]
        assert j[key]["value"] > 0 and j[key]["per_gpu_batch"] == 64 and 0 < j[key]["roofline"]["frac"] < 1, j[key]
    assert j["train_step"]["loss"] == j["train_step"]["loss"] and j["train_step"]["grad_norm"] > 0
    assert j["cfg4"]["roofline_attn_spatial"]["frac"] > 0 and j["cfg4"]["roofline_attn_temporal"]["frac"] > 0  # N = 36 / 1.5 rounds of 64-frame clips: two launches
    # 64 clips of 32 frames: the launch-time estimate gives the temporal layers to the small-tile in-projection + attention core (the
    # fused kernel's 192 items would leave a quarter of the CUs idle); either way the temporal core is timed against HBM (round-3
    # review: the leg printed 0 launches)
    sb_t = j["small_batch"]["roofline_attn_temporal"]
    assert sb_t["launches_per_step"] > 0 and sb_t["frac"] > 0, sb_t
    # 256 clips (this run's main line): the fused kernel, with the core alone still reported against HBM
    assert head["roofline_attn_temporal"]["frac"] > 0
    if os.environ.get("STLT_FUSED_MHSA") != "0":  # (a suite run with the fused kernel switched off keeps the two launches)
        assert head["roofline_mhsa_fused"]["frac"] > 0
    # the dense schedule beside `value` (how much of the headline is the exact elision of unread rows)
    ds = j["dense_schedule"]
    assert "error" not in ds and 0 < ds["value"] < head["value"] * 1.02 and ds["logit_max_abs_diff_vs_value_schedule"] <= 1e-5 and 0 < ds["roofline"]["frac"] < 1, ds
    # the reference's real layouts (T = layout_num_frames + 1): 33 x 8 and 17 x 5
    for key, tn in (("cfg2p", "T=33, N=8"), ("ref_default", "T=17, N=5")):
        assert "error" not in j[key] and tn in j[key]["workload"] and j[key]["value"] > 0 and 0 < j[key]["roofline"]["frac"] < 1, j[key]
    for key in ("cfg4", "small_batch"):  # the forward legs carry their own split-bf16 timing
        assert "error" not in j[key]["split_bf16"] and j[key]["split_bf16"]["value"] > 0 and j[key]["split_bf16"]["logit_max_abs_diff_vs_f32_forward"] <= 2e-4, j[key]["split_bf16"]
    assert "error" not in j["cfg5"]["split_bf16"] and j["cfg5"]["split_bf16"]["logit_max_abs_diff_vs_f32_forward"] <= 5e-4, j["cfg5"]["split_bf16"]
    assert "error" not in j["train_step"]["split_bf16"] and j["train_step"]["split_bf16"]["value"] > 0, j["train_step"]["split_bf16"]
    x3 = j["split_bf16"]  # the opt-in split-bf16 products ride beside `value` too (at 64 clips only the in-projections qualify)
    assert "error" not in x3 and x3["value"] > 0 and x3["gemm_tflops_f32_equivalent"] > 0 and x3["logit_max_abs_diff_vs_f32_forward"] <= 2e-4, x3


def test_two_rank_launch_line():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, STLT_BENCH_ONE_GPU="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), "bench.py", "--full", "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "64"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _last_json(r.stdout)
    assert REQUIRED <= set(j) and j["n_gpus"] == 2 and j["config"]["global_batch"] == 128 and j["value"] > 0
    assert "cpu_baseline" not in j  # rank 0 at N = 1 only
    assert j["ranks"]["world_size"] == 2 and len(j["ranks"]["ms_per_step_by_rank"]) == 2 and len(j["ranks"]["numa_pin_by_rank"]) == 2


def test_train_mode_single_process_line():
    r = subprocess.run([sys.executable, "bench.py", "--full", "--mode", "train", "--steps", "2", "--warmup", "1", "--batch", "8"], cwd=ROOT,
                       capture_output=True, text=True, timeout=900, env=dict(os.environ, STLT_BENCH_CPU_BUDGET_S="2"))
    assert r.returncode == 0, r.stderr[-2000:]
    j = _last_json(r.stdout)
    assert REQUIRED <= set(j) and j["n_gpus"] == 1 and j["value"] > 0 and "train step" in j["metric"]
    assert j["roofline"]["bound"] == "mfma" and j["roofline"]["flops_per_step"] > 0 and 0 < j["roofline"]["frac"] < 1
    assert j["cpu_baseline"]["value"] > 0 and j["cpu_baseline"]["kind"] == "port"
    assert j["loss"] == j["loss"] and j["grad_norm"] > 0  # finite


def test_train_mode_two_rank_launch_line():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, STLT_BENCH_ONE_GPU="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), "bench.py", "--full", "--mode", "train", "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "8"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _last_json(r.stdout)
    assert REQUIRED <= set(j) and j["n_gpus"] == 2 and j["config"]["global_batch"] == 16 and j["value"] > 0
    assert "all-reduce" in j["config"]["parallelism"] and "cpu_baseline" not in j
    assert j["ranks"]["world_size"] == 2 and len(j["ranks"]["ms_per_step_by_rank"]) == 2
    assert j["allreduce"]["ms_per_step_without_allreduce"] > 0  # the same steps without the gradient exchange, for the exposed time


@pytest.mark.parametrize("mode", ["forward", "train"])
def test_launch_bound_tool_prices_every_launch(mode):
    """tools/launch_bound.py (event-timed form; the rocprofv3 form is tools/collect_launch_bound.sh): one row per launch with the launcher's note,
    a bound and a ratio, and the step's sums."""
    if os.environ.get("STLT_GEMM16") == "0" or os.environ.get("STLT_GEMM_SPLIT_BF16", "0") != "0":
        pytest.skip("the table's expectations (small-tile products present, a note and a bound on every product) are the default dispatch's")
    r = subprocess.run([sys.executable, "tools/launch_bound.py", "--config", "cfg2", "--batch", "8", "--steps", "2", "--warmup", "3", "--mode", mode], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l.split() for l in r.stdout.splitlines() if l.strip() and l.strip()[0].isdigit()]
    assert len(rows) >= (80 if mode == "forward" else 150), len(rows)
    assert all(float(x[3]) > 0 for x in rows) and sum(x[2] != "-" for x in rows) >= len(rows) - 4
    notes = r.stdout
    assert "gemm16" in notes and "add_ln rows=" in notes and "M=" in notes and "ksteps=" in notes
    assert "(skinny)" in notes  # 8 clips: the one-row-per-clip tail runs as split-k partial tiles
    step = [l for l in r.stdout.splitlines() if l.startswith("# step:")][0]
    assert "achieved / bound" in step
