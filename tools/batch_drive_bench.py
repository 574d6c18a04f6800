"""Times driving a batch on the device (mgf_batch_set_forces, _apply_impulses, _copy_worlds) against the only routes there were before:
  (a) set_forces + apply_impulses on --bodies bodies of every world, one call each, against a whole-batch read_state, the same velocity
      update in numpy and a whole-batch write_state (that route cannot set a force or a torque at all: it is timed for the impulses alone);
  (b) copy_worlds of --copies worlds from a snapshot batch against one write_state call per world for the same worlds, from host arrays
      read beforehand (that route moves neither fat boxes, colliders nor constraint lists: it is the cheaper job).
K worlds of sphere_pile(8, 8, 8) after --ticks ticks, the snapshot after half of them.  Wall clock around the synchronous calls, the two
paths alternating in one process, every interval with a clock of its own, warm-up excluded, the median and the quartiles of --reps.
Before the timed rounds the copy is checked once on worlds that differ from their sources.  Run by hand; prints one JSON line per K."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgf_amd  # noqa: E402
from mgf_amd import scenes  # noqa: E402

STATE = ("x", "q", "v", "omega", "delta")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[256])
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--bodies", type=int, default=16, help="driven per world")
    ap.add_argument("--copies", type=int, default=64, help="worlds copied")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=31)
    a = ap.parse_args()
    ctx = mgf_amd.Context(0)
    sc = scenes.sphere_pile(8, 8, 8)
    dt, iters, n = float(sc["dt"]), sc["iters"], len(sc["comps"])
    for K in a.ks:
        b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
        snap = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
        snap.step(dt, iters, a.ticks // 2)
        b.step(dt, iters, a.ticks)
        rng = np.random.default_rng(1)
        world = np.repeat(np.arange(K, dtype=np.int32), a.bodies)
        body = np.concatenate([rng.choice(n, a.bodies, replace=False) for _ in range(K)]).astype(np.int32)
        order = rng.permutation(len(world))
        world, body = world[order], body[order]
        glob = world.astype(np.int64) * n + body
        force = rng.uniform(-5, 5, (len(world), 3)).astype(np.float32)
        torque = rng.uniform(-1, 1, (len(world), 3)).astype(np.float32)
        lin = rng.uniform(-1, 1, (len(world), 3)).astype(np.float32)
        ang = rng.uniform(-1, 1, (len(world), 3)).astype(np.float32)
        copies = min(a.copies, K)
        which = np.arange(copies, dtype=np.int32)
        snap_state = [snap.state(int(k)) for k in which]
        # the copy does something: the worlds differ from the snapshot before it and equal it directly behind it
        differed = any(not np.array_equal(b.state(int(k))["x"], snap_state[i]["x"]) for i, k in enumerate(which[:4]))
        b.copy_worlds(which, snap, which)
        same = all(np.array_equal(b.state(int(k))[f], snap_state[i][f]) for i, k in enumerate(which[:4]) for f in STATE)
        lists_same = all(b.constraints(int(k)).tobytes() == snap.constraints(int(k)).tobytes() for k in which[:4])
        t = dict(set_forces=[], apply_impulses=[], host_route=[], copy_worlds=[], write_states=[])
        launches = {}
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            b.set_forces(world, body, force, torque)
            t1 = time.perf_counter()
            launches["set_forces"] = b.counter("drive_launches")
            t2 = time.perf_counter()
            b.apply_impulses(world, body, lin, ang)
            t3 = time.perf_counter()
            launches["apply_impulses"] = b.counter("drive_launches")
            t4 = time.perf_counter()
            st = b.state()
            st["v"][glob] += lin            # (the bundled scene has mass 1; a sphere's inertia is a multiple of the identity)
            st["omega"][glob] += ang
            b.write_state(None, v=st["v"], omega=st["omega"])
            t5 = time.perf_counter()
            t5b = time.perf_counter()   # (the copy's own clock: not the end of the host route's)
            b.copy_worlds(which, snap, which)
            t6 = time.perf_counter()
            launches["copy_worlds"] = b.counter("drive_launches")
            t7 = time.perf_counter()
            for k, s in zip(which, snap_state):
                b.write_state(int(k), **s)
            t8 = time.perf_counter()
            if rep >= a.warmup:
                for key, v in dict(set_forces=t1 - t0, apply_impulses=t3 - t2, host_route=t5 - t4, copy_worlds=t6 - t5b, write_states=t8 - t7).items():
                    t[key].append(v)
        med = {k: 1e3 * float(np.median(v)) for k, v in t.items()}
        quart = {k: [round(1e3 * float(q), 4) for q in np.percentile(v, [25, 75])] for k, v in t.items()}
        print(json.dumps(dict(K=K, bodies_per_world=n, ticks=a.ticks, records=len(world), copies=int(copies),
                              set_forces_ms=med["set_forces"], apply_impulses_ms=med["apply_impulses"],
                              drive_ms=med["set_forces"] + med["apply_impulses"], host_route_ms=med["host_route"],
                              drive_speedup=med["host_route"] / (med["set_forces"] + med["apply_impulses"]),
                              copy_worlds_ms=med["copy_worlds"], write_states_ms=med["write_states"],
                              copy_speedup=med["write_states"] / med["copy_worlds"], drive_launches=launches, reps=a.reps, quartiles_ms=quart,
                              differed_before_copy=bool(differed), copied_state_equal=bool(same), copied_lists_equal=bool(lists_same))), flush=True)
        del b, snap
    ctx.close()


if __name__ == "__main__":
    main()
