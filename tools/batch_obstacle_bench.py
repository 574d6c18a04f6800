"""Times K small worlds with static Compound obstacles stepped as one batch (mgf_batch_step behind mgf_batch_set_world_obstacles)
against the same batch without obstacles and against K lone mgf_worlds given the same obstacles (mgf_world_add_obstacle) and stepped in
turn: K = 256 worlds of sphere_pile(8, 8, 8) - 512 spheres in a box - with two obstacles each, a ramp of three capsules with a ball on
its end and a ring of ten spheres, both entries of the table shared by all worlds, each world at poses of its own.  Wall clock around
synchronous calls (both paths drain the context's stream before they return), warm-up excluded, the median of repeated windows, as
tools/batch_bench.py takes it.  Run by hand; prints one JSON line: ms per tick of the batch with obstacles, of the batch without, of the
loop of lone worlds with obstacles, and the two ratios."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgf_amd  # noqa: E402
from mgf_amd import scenes  # noqa: E402


def windows(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def compounds():
    ramp = np.zeros(4, scenes.COMPONENT_DTYPE)
    ramp["tag"] = [1, 1, 1, 0]
    ramp["p"] = [(-3.0, 0.4, -1.0), (-3.0, 0.4, 0.0), (-3.0, 0.4, 1.0), (3.2, 0.9, 0.0)]
    ramp["d"] = [(6.0, 1.0, 0.0), (6.0, 1.0, 0.0), (6.0, 1.0, 0.0), (0, 0, 0)]
    ramp["r"] = [0.35, 0.35, 0.35, 0.8]
    ang = np.linspace(0.0, 2.0 * np.pi, 10, endpoint=False)
    ring = np.zeros(10, scenes.COMPONENT_DTYPE)
    ring["p"] = np.stack([2.5 * np.cos(ang), np.full(10, 0.5), 2.5 * np.sin(ang)], axis=1)
    ring["r"] = 0.55
    return ramp, ring


def poses(k):
    """world k's poses of the ramp and the ring: a turn about y and a small step of its own"""
    a, b = 0.05 * (k % 16), -0.04 * (k % 9)
    return (((0.02 * (k % 5), 0.2, -0.03 * (k % 7)), (float(np.cos(0.5 * a)), 0.0, float(np.sin(0.5 * a)), 0.0)),
            ((-0.03 * (k % 4), 0.0, 0.02 * (k % 6)), (float(np.cos(0.5 * b)), 0.0, float(np.sin(0.5 * b)), 0.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--window", type=int, default=20, help="ticks per timed window")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lone-window", type=int, default=3)
    ap.add_argument("--no-lone", action="store_true")
    a = ap.parse_args()
    ctx = mgf_amd.Context(0)
    K = a.k
    sc = scenes.sphere_pile(8, 8, 8)
    dt, iters, n = float(sc["dt"]), sc["iters"], len(sc["comps"])
    ramp, ring = compounds()

    def timed_batch(with_obstacles):
        b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
        if with_obstacles:
            ids = [b.add_obstacle(mgf_amd.Compound(ctx, c)) for c in (ramp, ring)]
            world = np.repeat(np.arange(K, dtype=np.int32), 2)
            ps = [p for k in range(K) for p in poses(k)]
            b.set_world_obstacles(world, np.tile(np.int32(ids), K), [p[0] for p in ps], [p[1] for p in ps])
        b.step(dt, iters, a.warmup)
        cons, static = [], []

        def window():
            st = b.step(dt, iters, a.window)
            cons.append(sum(s.n_constraints for s in st) / a.window)
            static.append(sum(s.n_terrain_constraints for s in st) / a.window)
        t = windows(window, a.reps) / a.window
        return t, float(np.median(cons)), float(np.median(static)), b.counter("launches_per_tick"), b.counter("capacity_retries")
    t_obs, c_obs, s_obs, launches, retries = timed_batch(True)
    t_plain, c_plain, s_plain, launches_plain, _ = timed_batch(False)
    row = dict(scene="sphere_pile", bodies_per_world=n, K=K, iters=iters, obstacles_per_world=2, batch_obstacles_ms_per_tick=1e3 * t_obs,
               batch_plain_ms_per_tick=1e3 * t_plain, obstacles_over_plain=t_obs / t_plain, constraints_per_tick=c_obs,
               static_constraints_per_tick=s_obs, plain_constraints_per_tick=c_plain, plain_static_constraints_per_tick=s_plain,
               launches_per_tick=launches, plain_launches_per_tick=launches_plain, capacity_retries=retries)
    if not a.no_lone:
        lone = []
        for k in range(K):
            w = mgf_amd.World.from_scene(ctx, sc)
            for comps, (disp, rot) in zip((ramp, ring), poses(k)):
                c = mgf_amd.Compound(ctx, comps)
                c.set_pose(disp, rot)
                w.add_obstacle(c)
            for _ in range(a.warmup):
                w.step(dt, iters)
            lone.append(w)
        lcons = []

        def lone_window():
            c = 0
            for _ in range(a.lone_window):
                for w in lone:
                    c += w.step(dt, iters).n_constraints
            lcons.append(c / a.lone_window)
        t_lone = windows(lone_window, a.reps) / a.lone_window
        row.update(lone_obstacles_ms_per_tick=1e3 * t_lone, lone_constraints_per_tick=float(np.median(lcons)), batch_speedup=t_lone / t_obs)
        del lone
    print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
