"""CPU: bench.py's rank-count contract, checked before any GPU call.

`--gpus N` under a launcher must equal the launcher's WORLD_SIZE (a line printed with the wrong
n_gpus would void a scaling run); the check runs before torch touches a device, so it is
testable here.
"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _run(args, **env):
    e = dict(os.environ, **env)
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args,
                          capture_output=True, text=True, timeout=120, env=e, cwd=REPO)


def test_gpus_mismatch_with_launcher_exits_nonzero():
    r = _run(["--gpus", "1", "--steps", "1"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 2, (r.returncode, r.stderr[-1000:])
    assert "WORLD_SIZE=2" in r.stderr
    r = _run(["--gpus", "8", "--steps", "1"], WORLD_SIZE="4", RANK="0", LOCAL_RANK="0")
    assert r.returncode == 2 and "--gpus 8" in r.stderr


def test_full_and_dump_outputs_options(monkeypatch):
    """A plain run is lean: --full is off unless asked for; --dump-outputs takes a folder."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_writes_float64_and_caps_its_size(tmp_path, monkeypatch):
    """dump_outputs on a stand-in for the step gather: small arrays whole, as float64; past the
    byte cap the same seeded sample on every call."""
    import numpy as np
    import torch

    import bench

    class Gather:
        gathered = None

        def __init__(self, t):
            self.t = t

        def last(self):
            return self.t

    sc = torch.arange(2 * 1000, dtype=torch.int32).reshape(2, 1000)
    bench.dump_outputs(str(tmp_path / "a"), Gather(sc))
    got = np.load(tmp_path / "a" / "scores.npy")
    assert got.dtype == np.float64 and np.array_equal(got, sc.numpy())
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 100)
    bench.dump_outputs(str(tmp_path / "b"), Gather(sc))
    bench.dump_outputs(str(tmp_path / "c"), Gather(sc))
    b, c = np.load(tmp_path / "b" / "scores.npy"), np.load(tmp_path / "c" / "scores.npy")
    assert 0 < b.size <= 100 and b.nbytes <= 800 and np.array_equal(b, c)
    assert np.all(np.diff(b) > 0)  # (values = flat indices here: ascending, no repeats)
    g = Gather(sc)
    g.gathered = [sc, sc + 1]
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 << 20)
    bench.dump_outputs(str(tmp_path / "d"), g)
    assert np.array_equal(np.load(tmp_path / "d" / "scores_rank1.npy"), sc.numpy() + 1.0)


def test_resolve_world_rules():
    import argparse
    import bench
    old = os.environ.pop("WORLD_SIZE", None)
    try:
        assert bench.resolve_world(argparse.Namespace(gpus=None)) == 1
        assert bench.resolve_world(argparse.Namespace(gpus=1)) == 1
        os.environ["WORLD_SIZE"] = "4"
        assert bench.resolve_world(argparse.Namespace(gpus=None)) == 4
        assert bench.resolve_world(argparse.Namespace(gpus=4)) == 4
    finally:
        os.environ.pop("WORLD_SIZE", None)
        if old is not None:
            os.environ["WORLD_SIZE"] = old
