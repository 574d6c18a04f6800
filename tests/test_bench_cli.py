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


class _TickWorld:
    """What bench.py's one-world lines drive of an mgf_amd.World (options, ticks, clones, counters), with fixed StepStats per tick."""

    def __init__(self, n_bodies=64):
        self.n = n_bodies

    def __len__(self):
        return self.n

    def set_option(self, key, value):
        pass

    def _tick(self):
        from mgf_amd._capi import StepStats
        return StepStats(n_bodies=self.n, n_constraints=100, n_pair_candidates=150, solver_kernel_launches=2, ms_solver_kernels=0.25,
                         ms_integrate=0.1, ms_broadphase=0.1, ms_narrowphase=0.1, ms_setup=0.1, ms_solve=0.5, ms_total=1.0)

    def step(self, dt, iters):
        return self._tick()

    def step_many(self, dt, iters, n):
        return [self._tick() for _ in range(n)]

    def clone(self):
        return _TickWorld(self.n)

    def counter(self, name):
        return 0


def _run_one_world(monkeypatch, capsys, argv):
    """bench.main() on a stand-in world: the JSON line it prints and which of the legs beyond the timed window it entered."""
    import json
    import torch
    import mgf_amd
    import bench
    entered = []

    def spy(name, fn=None, ret=None):
        def leg(*a, **k):
            entered.append(name)
            return fn(*a, **k) if fn else ret
        monkeypatch.setattr(bench, name, leg)
    spy("_instrumented_replays", bench._instrumented_replays)
    spy("bench_other_config", bench.bench_other_config)
    for name in ("order_deviation", "demo_order_cost", "cpu_baseline"):
        spy(name, ret={})
    small = lambda sc: sc.sphere_pile(4, 4, 4)  # noqa: E731  (configs 3 and 5's own scenes are large: their legs are what is counted here)
    for kind in ("config3", "config5"):
        monkeypatch.setitem(bench.OTHER_CONFIGS, kind, (bench.OTHER_CONFIGS[kind][0], small, bench.OTHER_CONFIGS[kind][2]))
    monkeypatch.setattr(mgf_amd, "Context", lambda dev: object())
    monkeypatch.setattr(mgf_amd.World, "from_scene", staticmethod(lambda ctx, scene: _TickWorld(len(scene["mass"]))))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--tile", "4", "4", "4", "--min-seconds", "0"] + argv)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MGF_RCCL_LIB", "MGF_BENCH_ALLOW_RCCL_OVERRIDE", "MGF_BENCH_DEVICE"):
        monkeypatch.delenv(k, raising=False)
    capsys.readouterr()
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), entered


HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def test_a_plain_run_times_its_window_and_nothing_else(monkeypatch, capsys):
    d, entered = _run_one_world(monkeypatch, capsys, ["--gpus", "1", "--steps", "6", "--warmup", "2"])
    assert entered == []
    assert all(k in d for k in HEADLINE) and d["metric"] == "contact_constraint_iters_per_sec" and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 6 and d["warmup"] == 2 and d["constraints_per_step"] == 100
    for extra in ("roofline", "phase_ms_per_step_rank0", "gpu_event_ms", "settled", "config3", "config5", "constraint_order_deviation", "cpu_baseline"):
        assert extra not in d, extra


def test_full_runs_every_leg_of_the_one_world_line(monkeypatch, capsys):
    d, entered = _run_one_world(monkeypatch, capsys, ["--gpus", "1", "--steps", "6", "--warmup", "2", "--full"])
    # the window's replays, the settled window's, then configs 3 and 5 each with their own replays; the order checks; the CPU baseline
    assert entered == ["_instrumented_replays", "order_deviation", "demo_order_cost", "_instrumented_replays",
                       "bench_other_config", "_instrumented_replays", "bench_other_config", "_instrumented_replays", "cpu_baseline"]
    assert all(k in d for k in HEADLINE) and d["steps"] == 6 and d["warmup"] == 2
    assert d["roofline"]["launches_timed"] == 12 and d["solver_launches_per_step"] == 2 and d["gpu_event_ms"]["replayed_window"] == 6.0
    assert d["settled"]["ms_per_step"] > 0 and d["settled"]["roofline"] and d["config3"]["roofline"] and d["config5"]["roofline"]
    assert d["cpu_baseline"] == {} and "constraint_order_deviation" in d


def test_the_other_configs_own_lines_replay_only_with_full(monkeypatch, capsys):
    d, entered = _run_one_world(monkeypatch, capsys, ["--scene", "config3", "--steps", "4"])
    assert entered == ["bench_other_config"] and "roofline" not in d and d["value"] > 0 and d["ms_per_step"] > 0
    d, entered = _run_one_world(monkeypatch, capsys, ["--scene", "config5", "--steps", "4", "--full", "--no-cpu-baseline"])
    assert entered == ["bench_other_config", "_instrumented_replays"] and d["roofline"]["launches_timed"] == 8
