"""bench.py's --gpus / WORLD_SIZE contract, checked before any GPU call (runs on CPU).

`python bench.py --gpus N` (N > 1) without a launcher starts the N ranks itself
(tests/test_gpu_bench.py::test_bench_gpus2_self_launch runs that on the GPU box); under a
launcher --gpus must equal WORLD_SIZE, otherwise the bench refuses to run."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, **env):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          timeout=120, cwd=ROOT, env=e)


def test_mismatched_gpus_exits_nonzero():
    out = _run(["--gpus", "2", "--steps", "1"], WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    assert out.returncode == 2, (out.returncode, out.stderr[-1000:])
    assert "WORLD_SIZE=3" in out.stderr and not out.stdout.strip()


def test_gpus_below_one_refused():
    out = _run(["--gpus", "0"])
    assert out.returncode != 0 and "--gpus must be >= 1" in out.stderr


def test_plain_and_full_options(monkeypatch):
    """--full is off by default; --dump-outputs takes a directory."""
    import bench
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_files_and_seeded_sample(tmp_path, monkeypatch):
    """bench.dump_outputs: float64 .npy per array (rank-suffixed at N > 1); above the size limit
    every array is cut to the same fixed, seeded sample of its elements, in index order."""
    import numpy as np
    import bench
    a = np.arange(1000, dtype=np.float32)
    b = np.arange(1000, 1040, dtype=np.float64).reshape(20, 2)
    bench.dump_outputs(str(tmp_path / "one"), {"a": a, "b": b, "none": None}, 1, 0)
    assert sorted(os.listdir(tmp_path / "one")) == ["a.npy", "b.npy"]
    la, lb = np.load(tmp_path / "one" / "a.npy"), np.load(tmp_path / "one" / "b.npy")
    assert la.dtype == lb.dtype == np.float64 and np.array_equal(la, a) and np.array_equal(lb, b)
    bench.dump_outputs(str(tmp_path / "two"), {"a": a}, 2, 1)
    assert os.listdir(tmp_path / "two") == ["a_rank1.npy"]
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8 * 200)   # 100 elements per array
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b}, 1, 0)
    s1, s2 = np.load(tmp_path / "s1" / "a.npy"), np.load(tmp_path / "s2" / "a.npy")
    assert s1.shape == (100,) and np.array_equal(s1, s2) and np.all(np.diff(s1) > 0) and set(s1) <= set(a)
    assert np.array_equal(np.load(tmp_path / "s1" / "b.npy"), b)   # already within its share


def test_launcher_command_shape():
    """The self-launch is ONE child torch.distributed.run with the script's own arguments and a
    127.0.0.1 rendezvous (the parent never initialises HIP, never execs)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert '"torch.distributed.run"' in src and '"--master-addr", "127.0.0.1"' in src
    assert "subprocess.Popen" in src and "os.exec" not in src
