"""bench.py's multi-rank path, end to end, on ONE GPU: two ranks launched exactly as the driver launches them
(python -m torch.distributed.run ... bench.py --gpus 2), sharing the device, with the collectives on gloo
(ADGS_BENCH_BACKEND=gloo: RCCL refuses two ranks on one GPU).  Not a measurement -- it guards the control flow (every rank must
issue the same collectives in the same order: settle windows, warm-up, timed steps, the final barrier) and the JSON contract."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


@pytest.mark.parametrize("config,exchange,world", [("T3", "factored", 2), ("T3", "dense", 2), ("C1", "factored", 2), ("T3", "factored", 4)])
def test_ranks_finish_and_print_one_json_line(config, exchange, world):
    env = dict(os.environ, ADGS_BENCH_BACKEND="gloo", ADGS_DP_EXCHANGE=exchange, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1", "--master-port",
           str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "6", "--warmup", "2", "--config", config, "--full"]
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=420)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == world and d["steps"] == 6 and d["warmup"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    assert abs(d["value"] - world * 6 / (d["ms_per_step"] * 6e-3)) / d["value"] < 1e-3          # whole-job frames / max-over-ranks time
    want = "factored" if (exchange == "factored" and config == "T3") else "dense"               # static configs have no raw-SH path
    assert d["config"]["gradient_exchange"].startswith(want), d["config"]["gradient_exchange"]
    # the self-verifying multi-GPU figures: the rank count the collective library itself reports, per-rank step times and pair
    # counts, the exchange under both forms of the dense reduction
    mg = d["config"]["multi_gpu"]
    assert mg["world_size"] == world and mg["rccl_ranks"] == world
    assert len(mg["per_rank_ms_per_step"]) == world and all(x > 0 for x in mg["per_rank_ms_per_step"])
    assert len(mg["per_rank_cell_pairs_last_frame"]) == world and all(x > 0 for x in mg["per_rank_cell_pairs_last_frame"])
    assert set(mg["exchange_ms_by_collective"]) == {"all_reduce", "rs_ag"}
    assert all(v is not None and v["total"] >= 0 and v["calls"] > 0 for v in mg["exchange_ms_by_collective"].values())
    assert d["config"]["camera_pool"].startswith("16 cameras")


@pytest.mark.parametrize("world,cams,densify,collective,self_launch", [(2, 3, 0, "all_reduce", False), (4, 3, 0, "rs_ag", False), (2, 5, 3, "rs_ag", True),
                                                                        (1, 3, 3, "all_reduce", False)])
def test_iteration_mode_cameras_per_iteration_densify_and_collective_forms(world, cams, densify, collective, self_launch):
    """BASELINE.json's C4 / C5 workloads on the small T3 scene: `cams` cameras per iteration dealt round-robin over the ranks
    (4 ranks x 3 cameras: one rank idles and still takes part in every collective), optional densify/prune inside the timed loop,
    both forms of the dense reduction, and `python bench.py --gpus N` starting its own ranks."""
    env = dict(os.environ, ADGS_BENCH_BACKEND="gloo", ADGS_DP_COLLECTIVE=collective, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    tail = ["--gpus", str(world), "--steps", "7", "--warmup", "2", "--config", "T3", "--cams-per-iter", str(cams), "--densify-every", str(densify)]
    if self_launch or world == 1:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + tail
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1", "--master-port",
               str(_free_port()), os.path.join(ROOT, "bench.py")] + tail
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == world and d["steps"] == 7 and d["scaling"] == "strong" and d["config"]["cameras_per_step"] == cams
    assert abs(d["value"] - cams * 7 / (d["ms_per_step"] * 7e-3)) / d["value"] < 1e-3          # cameras per second over the max-over-ranks time
    assert set(d["config"]["step_ms_hip_events"]) >= {"median", "p10", "p90"}
    if world > 1 or cams > 1:
        ex = d["config"]["exchange_ms"]
        assert ex["calls"] == 7 and ex["total"] >= 0 and {"allgather_wait", "expansion", "dense_reduction_wait"} <= set(ex)
    if densify:
        assert d["config"]["densify_ms"]["calls"] >= 7 // densify
        assert d["config"]["densify_ms"]["P_end"] > 0
    if collective == "rs_ag" and world > 1:
        assert "reduce-scatter" in d["config"]["gradient_exchange"]


@pytest.mark.parametrize("world,cams", [(2, 2), (3, 4), (3, 2), (3, 7)])
def test_multi_rank_training_loop_keeps_replicas_identical_and_matches_one_process(world, cams):
    """examples/train_dp.py (render -> losses -> backward -> factored exchange -> fused Adam -> densify/prune with a seeded sampler) as TWO
    or THREE ranks sharing the GPU (collectives on gloo) against ONE process accumulating the same cameras: every rank ends with
    bit-identical parameters, and the loss sequence of the multi-rank run follows the one-process run through the densification step.
    (3, 4): an uneven deal (2 + 1 + 1 cameras); (3, 2): one rank has NO camera in the iteration and still takes part in every collective."""
    env = dict(os.environ, ADGS_DP_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    args = ["--config", "T3", "--iters", "7", "--cams", str(cams), "--densify-every", "5"]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1", "--master-port",
                          str(_free_port()), os.path.join(ROOT, "examples", "train_dp.py")] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=420)
    assert two.returncode == 0, two.stderr[-2000:]
    assert "replicas identical: True" in two.stdout, two.stdout[-2000:]
    env1 = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    one = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_dp.py")] + args, env=env1, cwd=ROOT, capture_output=True, text=True, timeout=420)
    assert one.returncode == 0, one.stderr[-2000:]
    get = lambda out: [float(x) for x in [l for l in out.splitlines() if l.startswith("LOSSES ")][0].split()[1:]]
    a, b = get(two.stdout), get(one.stdout)
    assert len(a) == len(b) == 10
    assert all(abs(x - y) <= 2e-4 * abs(y) + 1e-7 for x, y in zip(a, b)), (a, b)
    size = lambda out: [l for l in out.splitlines() if "Gaussians at the end" in l][0].split(";")[1]
    assert size(two.stdout) == size(one.stdout)                       # the same rows were cloned / split / pruned


def _plain_run(config, steps, out_dir, extra=()):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "3", "--config", config,
           "--dump-outputs", str(out_dir)] + list(extra)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["ADGS_BENCH_DUMP_STEPS"] = "1000"                  # the per-step HIP-event series of the timed region, every step
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("config,extra", [("T3", []), ("C1", ["--graph", "on"])])
def test_plain_run_times_exactly_its_steps_and_dumps_the_last_step(config, extra, tmp_path):
    """A plain run (no --full): exactly --steps timed steps (one HIP-event interval each), the headline fields and nothing measured
    beside them, and with --dump-outputs what the last timed step returned, as float32 .npy files inside the 64 MB budget.  The timed
    region starts at pool entry 0 whatever the settle phase did: the last of 5 steps renders entry 4 of the 16-camera pool, the last
    of 21 steps entry 4 again (the same radii), the last of 6 steps entry 5 (other radii)."""
    import numpy as np
    out_dir = tmp_path / "dump"
    d = _plain_run(config, 5, out_dir, extra)
    assert d["metric"] == "fwd+bwd frames/s" and d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 5 and d["warmup"] == 3 and d["value"] > 0 and abs(d["value"] - 5 / (d["ms_per_step"] * 5e-3)) / d["value"] < 1e-3
    assert len(d["config"]["step_ms_series"]) == 5
    assert not {"roofline", "stages_ms", "cpu_baseline", "parity", "other_configs"} & set(d)
    dump = d["config"]["dumped_outputs"]
    assert dump["timed_step"] == 4 and [c["pool_entry"] for c in dump["cameras"]] == [4] and dump["cameras"][0]["camera"] == 4
    names = set(dump["arrays"])
    files = sorted(os.listdir(out_dir))
    assert files == sorted(n + ".npy" for n in names)
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64 << 20
    grads = [n for n in names if n.startswith("grad_") and n != "grad_means2D"]
    assert grads and all(np.load(out_dir / (n + ".npy")).dtype == np.float32 for n in names)
    assert all(np.isfinite(np.load(out_dir / (n + ".npy"))).all() for n in names)
    assert any(np.abs(np.load(out_dir / (n + ".npy"))).max() > 0 for n in grads)
    if extra:                                         # a graph replay returns the parameter gradients only
        assert names == set(grads)
        return
    assert {"color", "depth", "opacity", "flow", "semantic", "radii", "grad_means2D"} <= names
    assert np.load(out_dir / "color.npy").size == 3 * 208 * 320
    radii = np.load(out_dir / "radii.npy")
    same = _plain_run(config, 21, tmp_path / "same")
    assert len(same["config"]["step_ms_series"]) == 21 and same["config"]["dumped_outputs"]["cameras"][0]["pool_entry"] == 4
    assert np.array_equal(np.load(tmp_path / "same" / "radii.npy"), radii)
    other = _plain_run(config, 6, tmp_path / "other")
    assert len(other["config"]["step_ms_series"]) == 6 and other["config"]["dumped_outputs"]["cameras"][0]["pool_entry"] == 5
    assert not np.array_equal(np.load(tmp_path / "other" / "radii.npy"), radii)
