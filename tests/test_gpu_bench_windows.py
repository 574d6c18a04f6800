"""The benchmark's timed windows held to the oracle tick by tick, through mgf_world_step_many with default options.

Each window is rebuilt here from the scene builders bench.py uses, carried to its start the way bench.py carries it, and
snapshotted with mgf_world_clone as bench.py snapshots it.  The windows (keep them in step with bench.py):
  - config 2, transient: bench_single_world runs --warmup (10) single steps, clones, and times ticks 10..10+K.
  - config 2, settled: bench_single_world then steps the same world K (60) ticks and 400 - 10 - K more in two step_many calls,
    clones, and times ticks 400..400+K (the pile at rest: ~1 M constraints, mode 6's LDS plan at its narrow margins).
  - config 3: OTHER_CONFIGS["config3"], capsule_field(128, 32, 32, quads=158) at the default y0, step_many(150), ticks 150..150+K.
  - config 5: OTHER_CONFIGS["config5"], dumbbell_field(64, 16, 64), step_many(80), ticks 80..80+K.
Here T << K ticks of each window are checked (the oracle takes seconds per tick at these sizes).

Per window:
  1. the clone steps one tick per step_many(dt, iters, 1) call beside an oracle teacher-forced from the GPU's state at the window's
     start (x, q, v, omega, delta); every tick the state bits, the constraint counts and the constraint lists (impulses included)
     must agree.  n_pair_candidates is not compared: mgfo_world_set_state leaves the oracle's fat boxes from its own history.
  2. the world the clone was taken from steps the same T ticks in ONE step_many call (tick k + 1 enqueued before tick k is read
     back): its per-tick counts and its final state must be the oracle's.
  3. the path counters prove the ticks ran the kernels the bench times (and never a slow or retried path).  The sphere pile's pair
     search differs between its two windows: the falling pile runs k_pair_brick; in the settled pile too many queries fall outside the
     brick's staged box, k_pair_brick backs off (counter pair_brick_off_ticks counts down from a few hundred) and the window times
     k_pair_grid<true> - the same fused front end, each cell read from global memory."""
import time

import numpy as np
import pytest

from tests.util import compare_constraints, oracle_world, rel_err, values_equal

pytestmark = pytest.mark.gpu

FIELDS = ("x", "q", "v", "omega", "delta")

# name: (scene builder, how bench.py reaches the window's start: ("step" | "many", ticks) in order, T, constraint floor).
# T is sized by the oracle's time per tick (printed): ~6 s for the sphere pile, ~1.2 s for config 3, ~0.5 s for config 5.
WINDOWS = {
    "config2_transient": (lambda sc: sc.sphere_pile(64, 64, 64), [("step", 10)], 4, 400_000),
    "config2_settled": (lambda sc: sc.sphere_pile(64, 64, 64), [("step", 10), ("many", 60), ("many", 330)], 4, 900_000),
    "config3": (lambda sc: sc.capsule_field(128, 32, 32, quads=158), [("many", 150)], 10, 100_000),
    "config5": (lambda sc: sc.dumbbell_field(64, 16, 64), [("many", 80)], 16, 30_000),
}

PATH_COUNTERS = ("pair_brick_ticks", "front_rows_ticks", "fused_contacts_ticks", "early_cells_ticks", "pair_brick_off_ticks",
                 "capacity_retries", "row_overflows", "flow6_runs", "flow6_fallbacks", "solver_abort_fallbacks", "wide_ticks")


@pytest.fixture(scope="module")
def ctx():
    import mgf_amd
    c = mgf_amd.Context(0)
    yield c
    c.close()


def _counters(w):
    return {k: w.counter(k) for k in PATH_COUNTERS}


def _grew(before, after):
    return {k: after[k] - before[k] for k in PATH_COUNTERS if k != "pair_brick_off_ticks"}


def _check_path(name, w, before, T):
    """the T ticks since `before` ran the bench's kernels: no retried tick, no slow path, the block-local solver every tick"""
    after = _counters(w)
    d = _grew(before, after)
    assert d["capacity_retries"] == 0 and d["row_overflows"] == 0 and d["solver_abort_fallbacks"] == 0, (name, d)
    assert d["flow6_runs"] == T and d["flow6_fallbacks"] == 0, (name, d)
    if name == "config2_transient":  # spheres: the fused front end (k_contacts_spheres), k_pair_brick
        assert before["pair_brick_off_ticks"] == 0 and after["pair_brick_off_ticks"] == 0, (name, before, after)
        assert d["pair_brick_ticks"] == T and d["fused_contacts_ticks"] == T and d["front_rows_ticks"] == 0, (name, d)
    elif name == "config2_settled":  # ... with k_pair_grid<true>: k_pair_brick has backed off for longer than the window
        assert after["pair_brick_off_ticks"] == before["pair_brick_off_ticks"] - T > 0, (name, before, after)
        assert d["pair_brick_ticks"] == 0 and d["fused_contacts_ticks"] == T and d["front_rows_ticks"] == 0, (name, d)
    else:                            # capsules / two-part bodies: the list-free front end (k_pair_grid_n, k_front_rows.h)
        assert d["front_rows_ticks"] == T and d["pair_brick_ticks"] == 0 and w.counter("front_rows") == 1, (name, d)
        if name == "config3":        # the terrain side over the face grid: k_near_list, k_terrain_near, k_terrain_tests
            assert 0 < w.counter("front_slots") <= w.counter("front_faces"), (name, w.counter("front_slots"), w.counter("front_faces"))
    return d


def _multi_rows(cons):
    """rows that continue a manifold of several contacts (same body pair as the row before)"""
    ab = np.stack([cons["a"], cons["b"]], axis=1)
    return int(np.sum((ab[1:] == ab[:-1]).all(axis=1) & (ab[1:, 1] >= 0)))


@pytest.mark.parametrize("name", list(WINDOWS))
def test_bench_window_matches_oracle(ctx, name):
    import mgf_amd
    from mgf_amd import scenes
    build, route, T, floor = WINDOWS[name]
    scene = build(scenes)
    dt, iters = float(scene["dt"]), scene["iters"]
    world = mgf_amd.World.from_scene(ctx, scene)
    start = 0
    for how, k in route:
        if how == "step":
            for _ in range(k):
                world.step(dt, iters)
        else:
            world.step_many(dt, iters, k)
        start += k
    clone = world.clone()
    s0 = world.state()
    ow = oracle_world(scene)
    ow.set_state(**s0)
    assert all(values_equal(clone.state()[k], s0[k]) for k in FIELDS), "the clone does not hold the state it was taken from"

    # 1. tick by tick: the clone against the oracle
    cb = _counters(clone)
    want_counts, secs, multi = [], [], 0
    for t in range(T):
        sg = clone.step_many(dt, iters, 1)[0]
        t0 = time.perf_counter()
        so = ow.step(dt, iters)
        secs.append(time.perf_counter() - t0)
        want = (int(so.n_constraints), int(so.n_terrain_constraints))
        want_counts.append(want)
        got = (int(sg["n_constraints"]), int(sg["n_terrain_constraints"]))
        assert got == want, f"{name} tick {start + t}: (constraints, terrain) {got}, oracle {want}"
        oc = ow.constraints()
        compare_constraints(clone.constraints(), oc, check_impulse=True)
        multi = max(multi, _multi_rows(oc))
        g, o = clone.state(), ow.state()
        for k in FIELDS:
            assert values_equal(g[k], o[k]), f"{name} tick {start + t}: {k} not bit-identical (rel err {rel_err(g[k], o[k]):.3g})"
    dc = _check_path(name, clone, cb, T)
    assert dc["early_cells_ticks"] >= T - 1, (name, dc)  # (a clone's first tick has no last tick's box to lay its cells over)

    # 2. the same ticks pipelined in one call on the world the clone was taken from
    wb = _counters(world)
    many = world.step_many(dt, iters, T)
    got_counts = [(int(m["n_constraints"]), int(m["n_terrain_constraints"])) for m in many]
    assert got_counts == want_counts, f"{name}: step_many({T}) per-tick (constraints, terrain) {got_counts}, oracle {want_counts}"
    g, o = world.state(), ow.state()
    for k in FIELDS:
        assert values_equal(g[k], o[k]), f"{name}: step_many({T}) final {k} not bit-identical (rel err {rel_err(g[k], o[k]):.3g})"
    dw = _check_path(name, world, wb, T)
    assert dw["early_cells_ticks"] == T, (name, dw)  # (every pipelined tick laid its cells inside k_integrate)

    # 3. the window is what the bench times, not an emptied one
    assert min(c for c, _ in want_counts) > floor, (name, want_counts)
    if name in ("config3", "config5"):
        assert min(t for _, t in want_counts) > 0, (name, want_counts)
    if name == "config5":
        assert multi > 100, (name, multi)
    print(f"{name}: ticks {start}..{start + T}, oracle {np.mean(secs):.2f} s/tick, (constraints, terrain) per tick {want_counts}, "
          f"multi-contact rows {multi}, clone counters {dc}, pipelined counters {dw}")
