"""bench.py's multi-rank path: `--gpus N` spawns its own ranks; the sharded training workload
runs end to end (Env(shard=...), broadcast_model, gradient all-reduce, gather_costs for the
paired t-test, average_buffers).  On a one-GPU box the ranks share cuda:0 and the
collectives run over gloo (VRPGYM_BENCH_ONE_GPU=1, flagged in the JSON line)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _proc  # noqa: E402


# Ranks that SHARE cuda:0 (the one-GPU test aid; never the product's deployment): about one
# eight-rank start-up in sixty ended with "HSA_STATUS_ERROR_ILLEGAL_INSTRUCTION" in round 6, in a
# kernel of PyTorch's, not of this library.  A run is started ONCE: whatever ends
# it -- that abort included -- is the test's result, and nothing more is started on the GPU after
# a fault.


def _bench(args, extra_env=None, timeout=_proc.SUBPROCESS_TIMEOUT, env=None):
    """bench.py in a process group of its own that cannot outlive the test (tests/_proc.py; the
    launcher inside bench.py gives its ranks the same property).  One run, never repeated."""
    if env is None:
        env = dict(os.environ)
    env.update(extra_env or {})
    p = _proc.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, timeout=timeout)
    if p.returncode != 0:
        # the tail of a torchrun failure is its summary table; with VRPGYM_BENCH_LOG_DIR set the
        # whole stream is kept there, and the lines that name the cause go in front
        log_dir = os.environ.get("VRPGYM_BENCH_LOG_DIR")
        if log_dir:
            try:
                os.makedirs(log_dir, exist_ok=True)
                tag = "_".join(a.strip("-") for a in args)[:80]
                with open(os.path.join(log_dir, f"bench_stderr_{tag}.log"), "w") as fh:
                    fh.write(p.stderr)
            except OSError:
                pass
        cause = [l for l in p.stderr.splitlines()
                 if any(k in l for k in ("Error", "error", "HSA", "hip", "abort", "what():", "Assert"))
                 and "ChildFailedError" not in l][:30]
        p.stderr = "\n".join(cause) + "\n...\n" + p.stderr
    return p


def _json_line(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def test_bench_refuses_more_ranks_than_gpus():
    """--gpus N never silently benchmarks fewer ranks (round-1 verdict)."""
    if torch.cuda.device_count() >= 2:
        pytest.skip("two GPUs visible")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE")}
    env.pop("VRPGYM_BENCH_ONE_GPU", None)
    p = _proc.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, timeout=120)
    assert p.returncode != 0
    assert "--gpus 2" in p.stderr and "{" not in p.stdout


def test_bench_multirank_failure_is_one_loud_json_line():
    """N > 1, a rank dies during start-up (injected; first contact with RCCL will happen on the
    driver's 8-GPU node, never here): the launcher takes the other ranks down, exits non-zero and
    prints ONE JSON line with value null and an `error` field that names the rank, the stage and
    the exception (plus the tail of that rank's NCCL_DEBUG=WARN log when there is one)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(VRPGYM_BENCH_ONE_GPU="1", VRPGYM_BENCH_TEST_FAIL="startup:1")
    p = _proc.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1",
                   "--warmup", "1", "--no-cpu-baseline", "--no-north-star", "--no-extras"],
                  env=env, timeout=240)
    assert p.returncode != 0
    out = _json_line(p.stdout)
    assert out["value"] is None and out["n_gpus"] == 2 and out["ms_per_step"] is None
    assert "injected start-up failure" in out["error"] and "rank 1 [start-up]" in out["error"]
    assert 1 in out["failed_ranks"]
    assert "rank 1 failed in [start-up]" in p.stderr


def test_bench_rank0_reports_failure_under_torchrun():
    """Started the way the driver starts it (RANK / WORLD_SIZE already set: no launcher of ours),
    rank 0 itself owns the error line."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(port), VRPGYM_BENCH_ONE_GPU="1", VRPGYM_BENCH_TEST_FAIL="startup:0")
    env.pop("VRPGYM_BENCH_LAUNCHER", None)
    env.pop("VRPGYM_BENCH_FAILDIR", None)
    p = _proc.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1",
                   "--warmup", "1", "--no-cpu-baseline"], env=env, timeout=240)
    assert p.returncode != 0
    out = _json_line(p.stdout)
    assert out["value"] is None and "injected start-up failure" in out["error"]
    assert out["failed_ranks"] == [0]


def test_bench_distributed_timeout_is_bounded():
    """No collective of the bench waits longer than two minutes for a peer that is not there."""
    sys.path.insert(0, ROOT)
    import bench
    assert 0 < bench.DIST_TIMEOUT_S <= 120
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert src.count("init_process_group(") == src.count("timeout=tmo")


@pytest.mark.gpu
def test_bench_spawns_two_ranks_rollout():
    p = _bench(["--gpus", "2", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
                "--no-north-star", "--no-extras"], {"VRPGYM_BENCH_ONE_GPU": "1"})
    assert p.returncode == 0, p.stderr[:4000]
    out = _json_line(p.stdout)
    assert out["n_gpus"] == 2 and out["one_gpu_test_mode"] is True
    assert out["backend"] == "gloo" and out["rccl_ranks"] == 0 and len(out["devices"]) == 2
    d = out["dispersion"]
    assert d["ms_per_step_min"] <= d["ms_per_step_median"] <= d["ms_per_step_max"]
    assert d["rank_ms_per_step_min"] <= d["rank_ms_per_step_max"]
    assert out["config"]["global_batch"] == 1024 and out["config"]["steps_per_rollout"] == 19
    assert out["value"] > 0 and out["scaling"] == "weak"
    # rank 0 + rank 1 are the two halves of ONE seed-69 stream of 1024 graphs: their mean cost
    # is the mean cost of the unsharded 1024-graph batch only if the shards are disjoint rows
    # of that stream (scrambled masks differ per shard, so compare loosely)
    assert 6.0 < out["mean_tour_cost"] < 7.6


@pytest.mark.gpu
def test_bench_sharded_training_two_ranks():
    """configs[3]'s per-GPU shard with the all-reduce, t-test gather and buffer averaging."""
    p = _bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                "--workload", "irp40_b1024_train"], {"VRPGYM_BENCH_ONE_GPU": "1"})
    assert p.returncode == 0, p.stderr[:4000]
    out = _json_line(p.stdout)
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 2048
    tr = out["training"]
    assert tr["rollouts_per_step"] == 4          # 2 sampled + 2 greedy (baseline update)
    assert tr["grad_bucket_bytes"] == 4 * (1154944 - 128)   # IRP: _first_node has no gradient
    assert tr["allreduce_ms_per_step"] > 0
    assert out["value"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["tsp20_b512", "irp40_b1024_train"])
def test_bench_eight_ranks_one_gpu(workload):
    """The world size the driver's scaling run uses: port selection, eight shards of one
    seed-ordered stream, and for the training workload the 8-way gradient all-reduce, the 8-way
    gather_costs behind the paired t-test and average_buffers -- all ranks on cuda:0 over gloo
    (the rendezvous, sharding and collective CALL pattern are the real ones; RCCL is not)."""
    args = ["--gpus", "8", "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
            "--no-north-star", "--no-extras", "--workload", workload]
    p = _bench(args, {"VRPGYM_BENCH_ONE_GPU": "1"}, timeout=300)
    assert p.returncode == 0, p.stderr[:4000]
    out = _json_line(p.stdout)
    assert out["n_gpus"] == 8 and out["one_gpu_test_mode"] is True
    assert out["backend"] == "gloo" and len(out["devices"]) == 8
    B = 512 if workload == "tsp20_b512" else 1024
    assert out["config"]["global_batch"] == 8 * B
    assert out["value"] > 0 and out["mean_tour_cost"] == out["mean_tour_cost"]  # not NaN
    if workload.endswith("_train"):
        tr = out["training"]
        assert tr["rollouts_per_step"] == 4 and tr["allreduce_ms_per_step"] > 0
        assert tr["grad_bucket_bytes"] == 4 * (1154944 - 128)
    else:
        assert out["config"]["steps_per_rollout"] == 19
        assert 6.0 < out["mean_tour_cost"] < 7.6


def test_rank_binds_its_device_before_the_library_looks_at_it(monkeypatch):
    """bench.bind_device: set_device -> current_device check -> library census, in that order (a
    census taken before set_device would measure cuda:0 from every rank of a multi-GPU job)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import vrpgym_hip
    calls, state = [], {"dev": 0}
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: (calls.append(("set", d)), state.update(dev=d)))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: (calls.append(("cur",)), state["dev"])[1])
    monkeypatch.setattr(vrpgym_hip, "require_gpu", lambda: calls.append(("census", state["dev"])))
    dev = mod.bind_device(3)
    assert dev == torch.device("cuda", 3)
    assert calls[0] == ("set", 3) and calls[-1] == ("census", 3)
    assert ("cur",) in calls[1:-1]


def test_gpu_count_without_the_hip_runtime():
    """spawn_ranks counts GPUs in sysfs (KFD topology), never through HIP in the parent."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n = mod.visible_gpu_count()
    assert isinstance(n, int) and n >= 0
    print("GPUs counted without HIP:", n, "torch:", torch.cuda.device_count())
    if torch.cuda.is_available():
        assert n >= 1
    old = os.environ.get("HIP_VISIBLE_DEVICES")
    os.environ["HIP_VISIBLE_DEVICES"] = "0"
    try:
        assert mod.visible_gpu_count() <= 1
    finally:
        if old is None:
            del os.environ["HIP_VISIBLE_DEVICES"]
        else:
            os.environ["HIP_VISIBLE_DEVICES"] = old


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["tsp20_b512", "irp40_b1024_train"])
def test_bench_two_ranks_over_rccl(workload):
    """The real backend path, whenever the box has two GPUs: one process per GPU,
    dist.init_process_group("nccl") (= RCCL), distinct devices asserted inside bench.py, the
    rollout workload without a collective and the sharded training workload with the flat
    gradient all-reduce (ReduceOp.AVG, in place on the persistent bucket)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (the driver's 8-GPU node runs it)")
    args = ["--gpus", "2", "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
            "--no-north-star", "--no-extras", "--workload", workload]
    env = {k: v for k, v in os.environ.items() if k != "VRPGYM_BENCH_ONE_GPU"}
    p = _bench(args, env=env, timeout=120)
    assert p.returncode == 0, p.stderr[:4000]
    out = _json_line(p.stdout)
    assert out["n_gpus"] == 2 and out["rccl_ranks"] == 2 and out["backend"].startswith("nccl")
    assert "one_gpu_test_mode" not in out
    ids = {json.dumps({k: v for k, v in d.items() if k != "index"}, sort_keys=True) + str(d["index"])
           for d in out["devices"]}
    assert len(ids) == 2
    assert out["value"] > 0
    if workload.endswith("_train"):
        assert out["training"]["allreduce_ms_per_step"] > 0


@pytest.mark.gpu
def test_bench_plain_run_times_its_steps_and_dumps_outputs(tmp_path):
    """A plain run: the headline only (one block of exactly --steps steps, no extra runs), and
    --dump-outputs writes the last timed rollout's results -- the same in a second run."""
    got = []
    for i in range(2):
        d = tmp_path / f"out{i}"
        p = _bench(["--steps", "4", "--warmup", "1", "--dump-outputs", str(d)])
        assert p.returncode == 0, p.stderr[:4000]
        out = _json_line(p.stdout)
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in out, k
        assert out["steps"] == 4 and out["value"] > 0 and out["ms_per_step"] > 0
        for k in ("roofline", "other_configs", "cpu_baseline", "incl_env_reset", "dispersion"):
            assert k not in out, k
        # node-steps/s = B * N * T * steps / (steps * ms_per_step): one block of the 4 steps
        T = out["config"]["steps_per_rollout"]
        assert abs(out["value"] * out["ms_per_step"] / 1e3 / (512 * 20 * T) - 1) < 1e-2
        assert sorted(os.listdir(d)) == ["acc_logp.npy", "acc_loss.npy", "emb.npy", "notdone.npy"]
        arrs = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert all(a.dtype == np.float32 for a in arrs.values())
        assert arrs["acc_loss"].shape == (512,) and arrs["emb"].shape == (512, 20, 128)
        assert abs(-arrs["acc_loss"].mean() - out["mean_tour_cost"]) < 1e-4
        assert out["outputs"]["emb"] == {"shape": [512, 20, 128], "sampled": None}
        got.append(arrs)
    for k in got[0]:
        assert np.array_equal(got[0][k], got[1][k]), k


def test_dump_outputs_writes_float32_within_its_budget(tmp_path, monkeypatch):
    """bench.dump_outputs: float32 files (float64 kept), 0-d results included, and an array above
    its share of the budget written as a fixed, seeded, sorted sample of its elements."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_dump", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(mod, "DUMP_BYTES", 3 * 4096)
    big = torch.arange(10000, dtype=torch.float32).reshape(100, 100)
    outs = {"big": big, "ints": torch.arange(5, dtype=torch.int32), "loss": torch.tensor(2.5),
            "f64": torch.ones(3, dtype=torch.float64)}
    info = mod.dump_outputs(outs, str(tmp_path / "a"))
    mod.dump_outputs(outs, str(tmp_path / "b"))
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert a["ints"].dtype == np.float32 and a["ints"].tolist() == [0, 1, 2, 3, 4]
    assert a["loss"].dtype == np.float32 and float(a["loss"]) == 2.5
    assert a["f64"].dtype == np.float64
    assert info["big"] == {"shape": [100, 100], "sampled": 768} and a["big"].shape == (768,)
    assert np.all(np.diff(a["big"]) >= 0) and np.all(a["big"] == np.floor(a["big"]))
    assert np.array_equal(a["big"], np.load(tmp_path / "b" / "big.npy"))
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a")) <= 3 * 4096


@pytest.mark.gpu
def test_bench_single_rank_line_has_contract_keys():
    p = _bench(["--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-north-star", "--full"])
    assert p.returncode == 0, p.stderr[:4000]
    out = _json_line(p.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in out, k
    # `roofline` names the dominant kernel of the benched rollout: at TSP-20 x 512 the
    # one-launch encoder (fp32 MFMA-bound); the HBM-bound step kernel is roofline_step
    r = out["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us", "kernel"):
        assert k in r, k
    assert r["bound"] == "mfma" and r["kernel"] == "encoder_stack_x3_kernel<3>" and r["unit"] == "TFLOP/s"
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 2e-3
    # six bf16 MFMAs per fp32 product: the ceiling is priced on the bf16 matrix peak, and the
    # fraction can never exceed 1 (the figure against the fp32 MFMA peak is reported beside it)
    assert 157.3 < r["peak"] <= 2500.0 / 6 + 0.1 and 0 < r["frac"] < 1
    assert abs(r["issued_bf16_mfma_tflops"] / r["bf16_mfma_peak"] - r["frac"]) < 0.05
    assert r == {**out["roofline_encoder"], "share_of_rollout": r["share_of_rollout"]}
    r = out["roofline_step"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us",
              "loop_us_per_step", "loop_frac", "rollout_frac", "kernel"):
        assert k in r, k
    assert r["kernel"] == "decode_persistent_kernel" and r["bound"] == "hbm"
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["loop_frac"] <= r["frac"] + 1e-6 and r["rollout_frac"] <= r["loop_frac"] + 1e-6
    d = out["dispersion"]
    assert d["blocks"] == 5 and d["ms_per_step_min"] <= out["ms_per_step"] <= d["ms_per_step_max"]
    for name in ("vrp40_b2048_train", "irp40_b1024_train", "vrp100_b2048"):
        assert "error" not in out["other_configs"][name], out["other_configs"][name]
        assert out["other_configs"][name]["ms_per_step"] > 0


def test_failed_bench_run_is_never_started_again(monkeypatch, tmp_path):
    """The one-GPU aid runs a bench ONCE: a queue-error abort of ranks that share
    cuda:0 -- with or without a wave dump, in whichever code object -- and every other failure is
    the test's result; no tool library is put into the ranks' environment; the stream of a failed
    run lands in VRPGYM_BENCH_LOG_DIR when that is set."""
    class P:
        def __init__(self, rc, err):
            self.returncode, self.stderr, self.stdout = rc, err, ""
    abort = (":0:rocdevice.cpp :3676: Callback: Queue 0x1 aborting with error : "
             "HSA_STATUS_ERROR_ILLEGAL_INSTRUCTION")
    dump = ("wave_4: pc=0x78c7ede49a00 (kernel_code_entry=0x78c7ede49a80) (stopped, reason: "
            "ILLEGAL_INSTRUCTION)\nDisassembly:\n    code object: memory://1552#offset=0x64f5&"
            "size=3528496\n" + abort)
    script = []
    calls = []

    def fake_run(cmd, env=None, timeout=None):
        calls.append((cmd, dict(env or {})))
        return script.pop(0)
    monkeypatch.setattr(_proc, "run", fake_run)
    monkeypatch.delenv("VRPGYM_BENCH_LOG_DIR", raising=False)
    one = {"VRPGYM_BENCH_ONE_GPU": "1"}
    for rc, err in ((134, dump), (134, abort), (-6, abort), (139, "Segmentation fault"),
                    (1, "RuntimeError: something else")):
        n = len(calls)
        script[:] = [P(rc, err), P(0, "")]   # a second run would succeed: it must not happen
        p = _bench(["--gpus", "8"], dict(one))
        assert p.returncode == rc and len(calls) == n + 1 and len(script) == 1, (rc, err)
        assert err.splitlines()[-1] in p.stderr
        assert calls[-1][1].get("HSA_TOOLS_LIB") == os.environ.get("HSA_TOOLS_LIB")
    env = {k: v for k, v in os.environ.items() if k != "VRPGYM_BENCH_ONE_GPU"}
    script[:] = [P(134, dump), P(0, "")]    # one process per GPU: the same
    assert _bench(["--gpus", "8"], env=env).returncode == 134 and len(calls) == 6
    script[:] = [P(0, "")]
    assert _bench(["--steps", "3"]).returncode == 0 and len(calls) == 7
    assert not os.listdir(tmp_path)
    monkeypatch.setenv("VRPGYM_BENCH_LOG_DIR", str(tmp_path / "logs"))
    script[:] = [P(134, dump)]
    assert _bench(["--gpus", "8"], dict(one)).returncode == 134 and len(calls) == 8
    assert open(tmp_path / "logs" / "bench_stderr_gpus_8.log").read() == dump
