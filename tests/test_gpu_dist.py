"""GPU: the N > 1 path end to end on one card (two ranks, gloo): shard pack -> fused all-gather -> sharded ld_triangle."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.gpu
def test_two_ranks_one_card_sharded_triangle():
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), str(ROOT / "tests" / "_gpu_dist_worker.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GPU_DIST_OK" in r.stdout


@pytest.mark.gpu
def test_bench_launches_its_own_ranks():
    """The driver's command line, `python bench.py --gpus N`, without torch.distributed.run around it: the launcher starts
    the ranks as a child process and relays rank 0's line.  Two ranks share the one card here (gloo); the panel is small."""
    import json

    env = dict(os.environ, OMP_NUM_THREADS="1")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--snps", "3000",
                        "--backend", "gloo", "--settle-steps", "0", "--deadline", "400", "--full"], capture_output=True, text=True,
                       timeout=500, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["scaling"] == "strong"
    # a gloo rehearsal is NOT an RCCL run and must not read as one; both ranks sit on the one card
    assert rec["config"]["rccl_ranks"] is None and rec["config"]["group_ranks"] == 2 and rec["config"]["backend"] == "gloo"
    assert rec["config"]["nccl_version"] is None and rec["config"]["n_distinct_devices"] == 1
    assert rec["retried"] is False and rec["first_attempt_rc"] == 0
    assert rec["config"]["workload"] == "ld_triangle 3000x5008" and rec["value"] > 0
    assert rec["config"]["single_gpu_same_workload"]["pairs_per_s"] > 0
    assert rec["roofline"]["kernel_ms"] >= rec["roofline"]["kernel_ms_min_rank"] > 0
    # SURVEY 8(d) / VERDICT r05 item 4: the headline is the median of seven timed regions, all of them on the line
    assert len(rec["ms_per_step_runs"]) == 7 and rec["ms_per_step_min"] == min(rec["ms_per_step_runs"])
    assert rec["ms_per_step_min"] <= rec["ms_per_step"] and rec["ms_per_step"] == sorted(rec["ms_per_step_runs"])[3]
    # one record per rank
    assert [r_["rank"] for r_ in rec["per_rank"]] == [0, 1] and all(r_["kernel_ms"] > 0 and r_["pairs"] > 0 for r_ in rec["per_rank"])
    assert sum(r_["pairs"] for r_ in rec["per_rank"]) == 3000 * 2999 // 2


@pytest.mark.gpu
def test_bench_never_retries_a_wrong_result():
    """A rank whose timed steps do not reproduce the triangle ends the whole run with exit code 97: no second attempt, no
    JSON line (a retry there would hide exactly the class of bug the check exists for).  The hook
    --debug-corrupt-result flips one cell on rank 0 before the check."""
    env = dict(os.environ, OMP_NUM_THREADS="1")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--snps", "2000",
                        "--backend", "gloo", "--settle-steps", "0", "--deadline", "400", "--no-single-gpu-leg",
                        "--debug-corrupt-result", "--full"], capture_output=True, text=True, timeout=500, env=env, cwd=str(ROOT))
    assert r.returncode == 97, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert not any(ln.startswith("{") and '"metric"' in ln for ln in r.stdout.splitlines())
    assert "NOT retried" in r.stderr and "once more in the plainest mode" not in r.stderr


def _bench_n1(extra):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "3", "--warmup", "1", "--snps", "2000",
                           "--settle-steps", "0", "--no-cpu-baseline", "--other-scale", "small", "--full"] + extra,
                          capture_output=True, text=True, timeout=500, env=env, cwd=str(ROOT))


@pytest.mark.gpu
def test_bench_other_workloads_are_verified():
    """The N = 1 line's extra legs (configs[4] triangle, the configs[3] panel on one GPU, configs[2] ld_area, two streams)
    each compare their timed result with an independently computed one; the line must say they agreed."""
    import json

    r = _bench_n1([])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    legs = rec["other_workloads"]
    for key in ("ld_triangle 6000x1008", "ld_triangle 6000x1008, r2 only (2 B/pair)", "ld_triangle 12000x5008",
                "ld_area 12000 +-500kb r2>=0.8",
                "ld_triangle 6000x1008, 30 % of rows monomorphic", "ld_triangle 5000x5008, 0.1 % code-2 in 20 % of rows"):
        assert "error" not in legs[key], legs[key]
        assert legs[key]["results_equal"] is True, (key, legs[key])
    mono = legs["ld_triangle 6000x1008, 30 % of rows monomorphic"]
    assert 0.25 * 6000 < mono["non_ordinary_snps"]["acnt_zero_or_full"] < 0.35 * 6000 and mono["clean_twin_ms"] > 0
    assert 0.1 * 5000 < legs["ld_triangle 5000x5008, 0.1 % code-2 in 20 % of rows"]["non_ordinary_snps"]["with_missing_codes"] < 0.3 * 5000
    assert len(rec["ms_per_step_runs"]) == 7 and rec["ms_per_step_min"] <= rec["ms_per_step"]
    assert legs["ld_triangle 6000x1008"]["ms_min"] <= legs["ld_triangle 6000x1008"]["ms"]
    assert legs["ld_triangle 12000x5008"]["roofline"]["kernel_ms"] > 0
    assert "unit ranges [2, 7]" in legs["ld_triangle 12000x5008"]["verified_against"]
    assert rec["other_paths"]["two_streams"]["results_equal"] is True


@pytest.mark.gpu
def test_bench_a_wrong_extra_leg_is_a_failed_run():
    """a mismatch in an extra leg used to publish its throughput with exit code 0.  Now it ends the run like
    a mismatch of the headline: exit code 97, the marker line, no JSON line."""
    r = _bench_n1(["--debug-corrupt-other"])
    assert r.returncode == 97, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "BENCH_VERIFY_FAILED" in r.stdout and "ld_triangle 6000x1008" in r.stdout
    assert not any(ln.startswith("{") and '"metric"' in ln for ln in r.stdout.splitlines())


@pytest.mark.gpu
def test_bench_four_ranks_one_card_configs3():
    """VERDICT r04 item 4, as far as a box of this pool allows: at most six processes may have the card open at once, this
    test runner is one of them, and a run that exceeds the limit is killed (the eight-rank group therefore runs on the CPU,
    tests/test_dist_gloo.py).  `python bench.py --gpus 4 --backend gloo` on configs[3]'s panel, 100 000 x 5008 -- four
    ranks on cuda:0, UNEVEN slab shards (196, 196, 196, 194) packed per rank and exchanged through PanelPipeline, every
    rank's unit range verified cell for cell against the popcount kernel, the whole triangle timed on rank 0 alone beside
    it.  It is the code the driver runs on a multi-GPU node, with gloo in RCCL's place."""
    import json

    env = dict(os.environ, OMP_NUM_THREADS="1")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "4", "--steps", "2", "--warmup", "1", "--backend", "gloo",
                        "--settle-steps", "2", "--deadline", "800", "--full"], capture_output=True, text=True, timeout=900, env=env,
                       cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    cfg = rec["config"]
    assert rec["n_gpus"] == 4 and cfg["workload"] == "ld_triangle 100000x5008" and rec["scaling"] == "strong"
    assert cfg["group_ranks"] == 4 and cfg["rccl_ranks"] is None and cfg["backend"] == "gloo" and cfg["n_distinct_devices"] == 1
    assert rec["retried"] is False and rec["first_attempt_rc"] == 0
    assert "overlapped" in cfg["exchange"] and "popcount kernel" in cfg["launch"]
    assert cfg["single_gpu_same_workload"]["pairs_per_s"] > 0 and rec["value"] > 0
    # per rank its kernel time, the exposed part of its exchange and its share of the work.  The split is by
    # UNITS (8 rows x 128 columns: what the kernel's time is proportional to -- a unit on the diagonal or in the padding costs
    # what a full one costs), equal to within one unit; in PAIRS the last rank, which owns the short last tiles with their
    # larger share of diagonal units, therefore gets ~0.5 % fewer.
    pr = rec["per_rank"]
    assert [x["rank"] for x in pr] == [0, 1, 2, 3] and len(rec["ms_per_step_runs"]) == 7
    units = [x["units"] for x in pr]
    assert max(units) - min(units) <= 1
    pairs = [x["pairs"] for x in pr]
    assert sum(pairs) == 100000 * 99999 // 2 and max(pairs) / min(pairs) - 1.0 < 0.006, pairs
    assert all(x["kernel_ms"] > 0 and x["exchange_ms_per_step"] is not None for x in pr)


@pytest.mark.gpu
def test_bench_one_rank_rccl_group():
    """The sharded path over RCCL itself, as far as one card goes: `bench.py --force-dist` builds a ONE-rank nccl (= RCCL)
    process group and runs the shard pack -> all-gather -> unit-range kernel steps through it -- the code of an N-GPU run with
    N = 1.  The line must say it was an RCCL group, carry the seven timed regions and the per-rank record."""
    import json

    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--force-dist", "--steps", "3", "--warmup", "1", "--snps", "6000",
                        "--settle-steps", "2", "--no-cpu-baseline", "--no-other-workloads", "--no-extra-legs", "--full"],
                       capture_output=True, text=True, timeout=500, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    cfg = rec["config"]
    assert cfg["rccl_ranks"] == 1 and cfg["backend"] == "nccl" and cfg["nccl_version"] not in (None, "unknown")
    assert cfg["workload"] == "ld_triangle 6000x5008" and "popcount kernel" in cfg["launch"]
    assert len(rec["ms_per_step_runs"]) == 7 and rec["ms_per_step_min"] <= rec["ms_per_step"]
    assert len(rec["per_rank"]) == 1 and rec["per_rank"][0]["pairs"] == 6000 * 5999 // 2 and rec["per_rank"][0]["kernel_ms"] > 0


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full) times its K steps once and prints the headline only; --dump-outputs writes what the last
    timed step returned.  The same arguments give the same panel, so the FP4 kernel's dump and the popcount kernel's are
    equal value for value -- every pair of the 1 200-SNP triangle (fewer than bench.DUMP_PAIRS)."""
    import json

    import numpy as np

    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    for path in ("fp4", "popcount"):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "5", "--warmup", "2", "--snps", "1200",
                            "--path", path, "--dump-outputs", str(tmp_path / path)],
                           capture_output=True, text=True, timeout=300, env=env, cwd=str(ROOT))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert rec["steps"] == 5 and len(rec["ms_per_step_runs"]) == 1 and rec["ms_per_step"] == rec["ms_per_step_runs"][0] > 0
        assert rec["value"] > 0 and rec["higher_is_better"] is True and rec["config"]["workload"] == "ld_triangle 1200x5008"
        for key in ("cold_ms_per_step", "other_paths", "other_workloads", "cpu_baseline"):
            assert key not in rec, key
    names = sorted(f.name for f in (tmp_path / "fp4").iterdir())
    assert names == ["d_prime.npy", "int0.npy", "pairs.npy", "r_square.npy"]
    for name in names:
        a, b = np.load(tmp_path / "fp4" / name), np.load(tmp_path / "popcount" / name)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b, equal_nan=True), name
    pairs = np.load(tmp_path / "fp4" / "pairs.npy")
    assert pairs.shape == (1200 * 1199 // 2, 2) and np.all(pairs[:, 0] > pairs[:, 1])
    r2 = np.load(tmp_path / "fp4" / "r_square.npy")
    assert np.all((r2 >= 0) & (r2 <= 1)) and np.count_nonzero(r2) > 0
