"""bench.py's multi-GPU launch on the CPU: `--gpus N` starts N rank processes
itself (no torchrun), the ranks form a process group of N and rank 0 reports
the world size the group saw; a launcher whose world disagrees with --gpus is
refused.  `--dry-dist` stops before any GPU work, so gloo runs it here.
Also bench.py's options: a plain run prints the headline alone (`--full` adds
the rest) and `--dump-outputs` writes the last timed step's revenue exactly."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(cmd, env=None, timeout=180):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=e, cwd="/tmp")


@pytest.mark.parametrize("n", [2, 3])
def test_bench_spawns_n_ranks(n):
    p = _run([sys.executable, BENCH, "--gpus", str(n), "--dist-backend", "gloo", "--dry-dist"])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout                 # rank 0 alone prints
    d = json.loads(lines[0])
    assert d["n_gpus"] == n and d["world_size_seen"] == n
    assert d["rank_sum"] == n * (n - 1) // 2          # every rank joined the group
    assert d["dist_backend"] == "gloo"


def test_bench_single_rank_default():
    p = _run([sys.executable, BENCH, "--dry-dist"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(p.stdout.strip().splitlines()[-1])["n_gpus"] == 1


def test_bench_world_mismatch_refused():
    """torchrun with 2 ranks but --gpus 3: every rank exits non-zero."""
    p = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
              "--master-addr", "127.0.0.1", "--master-port", "29533", BENCH, "--gpus", "3",
              "--dist-backend", "gloo", "--dry-dist"])
    assert p.returncode != 0
    assert "process group has 2 ranks" in p.stderr


@pytest.mark.parametrize("revenue", [0, 1234567, (1 << 70) + 5, -3, (1 << 126) + (7 << 64) + (1 << 33) + 9])
def test_dump_outputs_revenue_exact(tmp_path, revenue):
    """--dump-outputs: the limbs restore the 128-bit revenue exactly."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    d = tmp_path / "out"
    bench.dump_outputs(str(d), revenue)
    assert sorted(p.name for p in d.iterdir()) == ["revenue.npy", "revenue_limbs32.npy"]
    v, limbs = np.load(d / "revenue.npy"), np.load(d / "revenue_limbs32.npy")
    assert v.dtype == np.float64 and v.shape == (1,) and v[0] == float(revenue)
    assert limbs.dtype == np.float64 and limbs.shape == (4,)
    u = sum(int(x) << (32 * i) for i, x in enumerate(limbs))
    assert (u - (1 << 128) if u >= (1 << 127) else u) == revenue


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(gdk, ora, tmp_path, monkeypatch, capsys):
    """A plain run (in this process, SF0.5) prints the headline alone, runs
    exactly --steps timed steps, and --dump-outputs holds the revenue of the
    line, which is the oracle's Q6 over the same generated rows."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    calls = []
    real = gdk.q6_fused
    monkeypatch.setattr(gdk, "q6_fused", lambda *a: calls.append(1) or real(*a))
    d = tmp_path / "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--sf", "0.5", "--steps", "3",
                                      "--warmup", "2", "--dump-outputs", str(d)])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    assert len(calls) == 5                           # warm-up + timed steps, nothing else
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert line["unit"] == "Grows/s" and line["higher_is_better"] is True and line["dtype"] == "int64"
    rows = line["config"]["rows_per_gpu"]
    # value = rows / ms_per_step, up to the rounding of both (3 and 4 decimals)
    ms = line["ms_per_step"]
    assert abs(line["value"] - rows / (ms * 1e-3) / 1e9) <= 1e-3 + line["value"] * 1e-4 / ms
    assert not {"roofline", "parity", "cpu_baseline", "q1", "config1_thetaselect"} & set(line)
    want = ora.q6(ora.tpch_lineitem(bench.SEED, 0, rows, max(1, int(0.5 * 200_000))), 1)
    assert int(line["revenue"]) == want
    limbs = np.load(d / "revenue_limbs32.npy")
    assert sum(int(x) << (32 * i) for i, x in enumerate(limbs)) == want
    assert np.load(d / "revenue.npy")[0] == float(want)


def test_bench_options():
    """A plain run is the default; --full and --dump-outputs are there;
    --steps 0 is refused (it could time nothing)."""
    p = _run([sys.executable, BENCH, "--help"])
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout
    p = _run([sys.executable, BENCH, "--steps", "0"])
    assert p.returncode == 2 and "--steps" in p.stderr


def test_pair_hash_order_sensitive():
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    a = np.arange(10, dtype=np.uint64)
    b = a[::-1].copy()
    h = bench._pair_hash(a, b, 0)
    # split into two ranks' slices: the sum of the parts is the whole
    assert (bench._pair_hash(a[:4], b[:4], 0) + bench._pair_hash(a[4:], b[4:], 4)) % (1 << 64) == h
    # swapping two pairs changes it
    a2, b2 = a.copy(), b.copy()
    a2[[2, 3]] = a2[[3, 2]]
    b2[[2, 3]] = b2[[3, 2]]
    assert bench._pair_hash(a2, b2, 0) != h
