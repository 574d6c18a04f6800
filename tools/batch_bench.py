"""Times K small worlds stepped as one batch (mgf_batch_step) against the same K scenes as K lone mgf_worlds on one context stepped in
turn - the only way to do that job without a batch - for K worlds of balls_demo(8) at a settled window and of sphere_pile(8, 8, 8) from
tick 0.  Wall clock around synchronous calls (both paths drain the context's stream before they return), warm-up excluded, the median
of repeated windows as bench.py takes it.  Run by hand; prints one JSON line per (scene, K):
  K, ms per tick of the batch, ms per tick of the loop of lone worlds, world-ticks per second and constraint-iterations per second of both.
The lone worlds of the settled scene start from the batch's state at the end of its settling ticks (positions, velocities, motion),
so that both paths time the same pile; --lone-max bounds the K up to which the loop is run at all (K worlds are K sets of device arrays).
--own-terrain says what the worlds of the batch stand on: `shared` - one mesh for all (mgf_batch_set_terrain); `offset` - one entry of
the terrain table, every world at a position of its own (the scene's bodies moved along, so that every world does the same work);
`distinct` - K entries: K copies of the scene's mesh, or for capsule_field K heightfields of K seeds (the lone loop is not run then:
its worlds would not be the batch's).  The scene capsule_field is capsule_field(8, 4, 8): 256 capsules over a heightfield."""
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


def world_scenes(name, K, own):
    """the K scenes of a batch"""
    if name == "balls_demo":
        sc = scenes.balls_demo(8)
    elif name == "capsule_field":
        sc = scenes.capsule_field(8, 4, 8)
    else:
        sc = scenes.sphere_pile(8, 8, 8)
    if own == "shared":
        return [sc] * K
    if own == "offset":   # the whole world moved by a step of its own: the same work everywhere, K positions of one mesh
        out = []
        for k in range(K):
            off = np.float32([0.37 * (k % 32), 0.11 * (k // 32), -0.23 * (k % 7)])
            comps = sc["comps"].copy()
            comps["p"] = (comps["p"] + off).astype(np.float32)
            out.append(dict(sc, comps=comps, terrain=dict(sc["terrain"], pos=(np.asarray(sc["terrain"]["pos"], np.float32) + off).astype(np.float32))))
        return out
    if name == "capsule_field":
        return [scenes.capsule_field(8, 4, 8, seed=1000 + k) for k in range(K)]
    out = []
    for k in range(K):   # K meshes that differ in one vertex far below the scene by an amount that moves no contact: K table entries
        verts = np.array(sc["terrain"]["verts"], np.float32)
        verts = np.concatenate([verts, np.float32([[0.0, -1000.0 - k, 0.0]])])
        out.append(dict(sc, terrain=dict(sc["terrain"], verts=verts)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 16, 256, 1024, 4096])
    ap.add_argument("--scenes", nargs="+", default=["balls_demo", "sphere_pile"])
    ap.add_argument("--settle", type=int, default=300, help="ticks before the timed windows of balls_demo")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--window", type=int, default=20, help="ticks per timed window")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lone-max", type=int, default=1024)
    ap.add_argument("--lone-window", type=int, default=5)
    ap.add_argument("--own-terrain", choices=["shared", "offset", "distinct"], default="shared")
    a = ap.parse_args()
    ctx = mgf_amd.Context(0)
    for name in a.scenes:
        own = a.own_terrain
        sc = world_scenes(name, 1, "shared")[0]
        dt, iters, n = float(sc["dt"]), sc["iters"], len(sc["comps"])
        settle = a.settle if name == "balls_demo" else 0
        for K in a.ks:
            scs = world_scenes(name, K, own)
            b = mgf_amd.WorldBatch.from_scenes(ctx, scs) if own == "shared" else mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
            if settle:
                b.step(dt, iters, settle)
            start = b.state() if K <= a.lone_max else None
            b.step(dt, iters, a.warmup)
            cons = []

            def batch_window():
                st = b.step(dt, iters, a.window)
                cons.append(sum(s.n_constraints for s in st) / a.window)
            t_batch = windows(batch_window, a.reps) / a.window
            row = dict(scene=name, bodies_per_world=n, K=K, iters=iters, settle_ticks=settle, batch_ms_per_tick=1e3 * t_batch,
                       batch_world_ticks_per_s=K / t_batch, constraints_per_tick=float(np.median(cons)),
                       batch_constraint_iters_per_s=float(np.median(cons)) * iters / t_batch, launches_per_tick=b.counter("launches_per_tick"),
                       capacity_retries=b.counter("capacity_retries"))
            if own != "shared":
                row.update(own_terrain=own, terrain_entries=b.terrain_count())
            del b
            if K <= a.lone_max and own == "shared":
                lone = [mgf_amd.World.from_scene(ctx, sc) for _ in range(K)]
                for k, w in enumerate(lone):
                    if settle:
                        w.write_state(**{f: start[f][k * n:(k + 1) * n] for f in ("x", "q", "v", "omega", "delta")})
                    for _ in range(a.warmup):
                        w.step(dt, iters)
                lcons = []

                def lone_window():
                    c = 0
                    for _ in range(a.lone_window):
                        for w in lone:
                            c += w.step(dt, iters).n_constraints
                    lcons.append(c / a.lone_window)
                t_lone = windows(lone_window, a.reps) / a.lone_window
                row.update(lone_ms_per_tick=1e3 * t_lone, lone_world_ticks_per_s=K / t_lone, lone_constraints_per_tick=float(np.median(lcons)),
                           lone_constraint_iters_per_s=float(np.median(lcons)) * iters / t_lone, batch_speedup=t_lone / t_batch)
                del lone
            print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
