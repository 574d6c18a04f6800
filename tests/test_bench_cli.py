"""bench.py's launcher half (no GPU): `python bench.py --gpus N` issued like the N = 1 command becomes the launcher of its own N ranks
(it used to raise SystemExit, and a scaling run issued that way would have recorded rc != 0 at every N > 1)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _run_main(monkeypatch, argv, env=None):
    import subprocess
    import bench
    calls = []
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None: calls.append((cmd, env)) or 0)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MGF_RCCL_LIB", "MGF_BENCH_ALLOW_RCCL_OVERRIDE", "MGF_BENCH_DEVICE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        bench.main()
    except SystemExit as e:
        return calls, e.code
    return calls, None


def test_gpus_n_without_a_launcher_spawns_the_ranks(monkeypatch):
    calls, code = _run_main(monkeypatch, ["--gpus", "4", "--steps", "7", "--warmup", "3"])
    assert code == 0 and len(calls) == 1
    cmd, env = calls[0]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    k = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[k + 1:] == ["--gpus", "4", "--steps", "7", "--warmup", "3"]   # the ranks get the command line as it was given
    assert env["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_the_stand_in_transport_puts_the_ranks_on_one_device(monkeypatch, tmp_path):
    lib = tmp_path / "libfake.so"
    lib.write_bytes(b"")
    calls, code = _run_main(monkeypatch, ["--gpus", "2", "--scene", "config5", "--rccl-lib", str(lib)])
    assert code == 0
    cmd, env = calls[0]
    assert env["MGF_BENCH_DEVICE"] == "0" and cmd[-2:] == ["--backend", "gloo"]   # (this container has no device at all: fewer than 2)


def test_a_mismatched_launcher_is_refused(monkeypatch):
    calls, code = _run_main(monkeypatch, ["--gpus", "4"], env={"WORLD_SIZE": "2", "RANK": "0"})
    assert not calls and "WORLD_SIZE=2" in str(code)


class _FakeWorld:
    """What dump_outputs reads of a world (mgf_amd.World's state / constraints / tags), filled with seeded numbers."""

    def __init__(self, n_bodies, n_constraints, seed):
        from mgf_amd._capi import CONSTRAINT_DTYPE
        import numpy as np
        rng = np.random.default_rng(seed)
        self.st = {k: rng.standard_normal((n_bodies, d)).astype(np.float32) for k, d in (("x", 3), ("q", 4), ("v", 3), ("omega", 3), ("delta", 3))}
        self.cons = np.zeros(n_constraints, CONSTRAINT_DTYPE)
        self.cons["a"] = np.arange(n_constraints)
        self.cons["normal"] = rng.standard_normal((n_constraints, 3))
        self.cons["normal_impulse"] = rng.standard_normal(n_constraints)

    def state(self):
        return self.st

    def constraints(self):
        return self.cons

    def tags(self):
        import numpy as np
        return np.arange(len(self.st["x"]), dtype=np.uint32)[::-1].copy()


def _stats(n):
    import bench
    return {k: n + i for i, k in enumerate(bench.DUMP_STAT_KEYS)}


def test_dump_outputs_writes_the_whole_of_a_small_world(tmp_path):
    import numpy as np
    import bench
    w = _FakeWorld(100, 40, 1)
    bench.dump_outputs(str(tmp_path), [("", w, None)], [_stats(100)])
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    for k in ("x", "q", "v", "omega", "delta"):
        assert np.array_equal(got[k], w.st[k])
    assert np.array_equal(got["body_rows"], np.arange(100)) and np.array_equal(got["constraint_rows"], np.arange(40))
    assert np.array_equal(got["constraint_a"], np.arange(40)) and got["constraint_a"].dtype == np.float64
    assert np.array_equal(got["constraint_normal"], w.cons["normal"]) and np.array_equal(got["constraint_normal_impulse"], w.cons["normal_impulse"])
    assert list(got["step_stats"]) == [100 + i for i in range(len(bench.DUMP_STAT_KEYS))]
    assert "tags" not in got


def test_dump_outputs_samples_large_outputs_the_same_way_every_time_within_64_mb(tmp_path):
    import numpy as np
    import bench
    worlds = [(f"tile{t}_", _FakeWorld(40000, 30000, t), t) for t in range(8)]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), worlds, [_stats(40000)] * 8)
    a = {p.name: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    b = {p.name: np.load(p) for p in (tmp_path / "b").glob("*.npy")}
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy")) <= 64 << 20
    rows = a["tile3_body_rows.npy"].astype(np.int64)
    assert len(rows) == bench.DUMP_BODY_ROWS // 8 and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["tile3_x.npy"], worlds[3][1].st["x"][rows]) and np.array_equal(a["tile3_tags.npy"], worlds[3][1].tags()[rows])
    assert len(a["tile3_constraint_rows.npy"]) == bench.DUMP_CONSTRAINT_ROWS // 8
    assert not np.array_equal(rows, a["tile4_body_rows.npy"])   # (each tile its own sample)


def test_dump_outputs_of_the_largest_single_world_stays_within_64_mb(tmp_path):
    import bench
    w = _FakeWorld(2 * bench.DUMP_BODY_ROWS, 3 * bench.DUMP_CONSTRAINT_ROWS, 2)
    bench.dump_outputs(str(tmp_path), [("", w, None)], [_stats(1)])
    assert sum(p.stat().st_size for p in tmp_path.glob("*.npy")) <= 64 << 20
