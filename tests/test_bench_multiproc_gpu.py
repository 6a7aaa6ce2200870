"""GPU (one device is enough): the N > 1 script path of bench.py executed end to end by TWO real processes under torch.distributed.run --
rendezvous over gloo on 127.0.0.1, the 128-byte RCCL id made and broadcast, per-rank engines, barriers, EXACTLY K timed steps, max-over-ranks
clock, ONE JSON line on rank 0 -- with DQN_BENCH_SIM_COMM=1: both ranks share GPU 0 and each engine runs the data-parallel step program
(DQN_SIM_WORLD = 2: two half graphs, pack, wide dW over 2 x B gathered samples, sum over ranks, Adam with g / world) with the all-gather
replaced by local copies, because RCCL refuses two ranks on one device.  Only ncclCommInitRank / ncclAllGather are not executed (they are at
world 1 in tests/test_dp_gpu.py).  VERDICT r02 item 4b: the driver's --gpus N launch must not meet this code path for the first time."""
import json
import os
import socket
import subprocess
import sys

import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("launcher", ["torchrun", "self"])
def test_bench_two_ranks_script_path(launcher):
    """launcher = torchrun: the form the driver uses for N > 1; self: plain `python bench.py --gpus 2` (no WORLD_SIZE), which re-execs itself under
    torch.distributed.run on a free loopback port and propagates the return code"""
    env = dict(os.environ, DQN_BENCH_SIM_COMM="1", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    bench_args = ["--gpus", "2", "--steps", "6", "--warmup", "3", "--replay", "512", "--env-steps", "8", "--profile-steps", "1", "--sustained-steps", "40", "--cpu-seconds", "1", "--full"]
    if launcher == "torchrun":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
               os.path.join(ge.ROOT, "bench.py")] + bench_args
    else:
        cmd = [sys.executable, os.path.join(ge.ROOT, "bench.py")] + bench_args
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ge.ROOT)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]                 # rank 0 prints ONE JSON line, rank 1 none
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 6 and d["warmup"] == 3 and d["scaling"] == "weak" and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["value"] - 2 * 6 / (d["ms_per_step"] * 6e-3)) < 1e-6 * d["value"]      # whole-job rate = world x K / max-over-ranks time
    assert d["config"]["global_batch"] == 64 and d["config"]["workload"].startswith("configs[2]") and "sim_comm" in d["config"]
    assert d["roofline"]["traffic"] is None                   # the committed PMC passes are single-GPU runs: not quoted for a replica step
    assert d["cpu_baseline"] is not None and d["cpu_baseline"]["value"] > 0          # rank 0 keeps the CPU baseline at N > 1
    assert d["sustained"]["steps"] == 40 and d["sustained"]["value"] > 0
    assert d["env_loop"]["act_only_env_steps_per_s"] > 0
    # the line says what the communicator saw: here (self-test, no ncclCommInitRank) nothing -- on a real N-GPU launch bench.py asserts rccl_nranks == WORLD_SIZE
    assert d["config"]["rccl_nranks"] == 0 and d["config"]["rccl_rank"] == -1 and d["config"]["exchange"].startswith("all-gather") and d["config"]["dp_overlap"] is False
    assert d["per_call"] is None                              # the per-call seam is a single-device measurement


def test_bench_single_gpu_line_fields():
    """the --full single-GPU line carries per_call (sync + async seam), a sustained region sized in seconds and a dominant kernel named from the committed profile"""
    cmd = [sys.executable, os.path.join(ge.ROOT, "bench.py"), "--steps", "20", "--warmup", "5", "--replay", "2048", "--env-steps", "0", "--profile-steps", "2",
           "--sustained-seconds", "0.5", "--no-cpu-baseline", "--full"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ge.ROOT)
    assert p.returncode == 0, p.stderr[-4000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    pc = d["per_call"]
    assert pc["sync"]["calls"] == pc["async"]["calls"] == 20 and pc["sync"]["value"] > 0 and pc["async"]["value"] >= 0.9 * pc["sync"]["value"]
    assert 0.3 < d["sustained"]["seconds"] < 2.0 and d["sustained"]["steps"] >= 1000
    dk = d["roofline"]["dominant_kernel"]
    assert dk["rocprof_file"].startswith("profiles/") and dk["kernel"] in dk["rocprof_symbol"] and dk["bound"] in ("mfma", "hbm") and 0 < dk["frac"] < 1
    assert d["config"]["rccl_nranks"] == 0 and d["config"]["exchange"] == "none"


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """a plain run (no --full) prints the headline alone; --dump-outputs writes the timed call's last-step outputs as float32 / float64 .npy files,
    the same from run to run with the same arguments"""
    import numpy as np
    runs = []
    for i in range(2):
        cmd = [sys.executable, os.path.join(ge.ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3", "--replay", "512", "--dump-outputs", str(tmp_path / str(i))]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ge.ROOT)
        assert p.returncode == 0, p.stderr[-4000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        runs.append(json.loads(lines[0]))
    d = runs[0]
    assert d["steps"] == 7 and d["warmup"] == 3 and d["unit"] == "steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    for k in ("roofline", "cpu_baseline", "env_loop", "sustained", "per_call", "secondary"):
        assert k not in d, k
    names = sorted(f.name for f in (tmp_path / "0").iterdir())
    assert names == sorted(f.name for f in (tmp_path / "1").iterdir()) and "params_online.npy" in names and "loss.npy" in names
    assert sum((tmp_path / "0" / n).stat().st_size for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(tmp_path / "0" / n), np.load(tmp_path / "1" / n)
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), n
        np.testing.assert_array_equal(a, b, err_msg=n)
    assert np.load(tmp_path / "0" / "loss.npy")[0] == np.float32(d["config"]["last_loss"])
    assert np.load(tmp_path / "0" / "params_online.npy").size == d["config"]["n_params"]
