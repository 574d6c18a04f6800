"""Times the world queries (mgf_world_raycast_many, mgf_world_sweep_many, mgf_world_overlap_aabb_many) on BASELINE config 2's scene
(262 144 spheres) after 20 ticks: 65 536 particles - half rays, half segments - aimed into the pile, 65 536 casts - half spheres,
half capsules, swept from zero to several cells - aimed into the pile as the rays are, and 16 384 boxes one to four body widths
wide.  The grid build and the query pass are timed with HIP events inside the call (mgf_world_counter "query_build_ns" /
"query_run_ns"); the wall time of the whole call (uploads and read-backs included) beside them.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgf_amd  # noqa: E402
from mgf_amd import scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--casts", type=int, default=65536)
    ap.add_argument("--boxes", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    ctx = mgf_amd.Context(0)
    sc = scenes.config(1)
    w = mgf_amd.World.from_scene(ctx, sc)
    w.step_many(float(sc["dt"]), sc["iters"], a.ticks)
    cen = w.colliders()["p"]
    lo, hi = cen.min(axis=0), cen.max(axis=0)
    rng = np.random.default_rng(0)
    tgt = rng.uniform(lo, hi, (a.rays, 3))
    p = tgt + rng.normal(0.0, 1.0, (a.rays, 3)) * (hi - lo) * 0.25 + np.array([0.0, (hi - lo)[1], 0.0])
    d = (tgt - p).astype(np.float32)
    dt = np.where(np.arange(a.rays) % 2 == 0, np.float32(np.inf), np.float32(1.0)).astype(np.float32)
    # casts: radius 0.2-0.6, capsules 0.3-1.5 long, from a point above the pile towards one in it, swept 0-6 units (cells are ~1 wide)
    ctgt = rng.uniform(lo, hi, (a.casts, 3))
    csrc = ctgt + rng.normal(0.0, 1.0, (a.casts, 3)) * 2.0 + np.array([0.0, 3.0, 0.0])
    dirn = (ctgt - csrc) / np.linalg.norm(ctgt - csrc, axis=1, keepdims=True)
    casts = np.zeros(a.casts, mgf_amd.MOVING_DTYPE)
    casts["tag"] = np.arange(a.casts) % 2
    casts["r"] = rng.uniform(0.2, 0.6, a.casts)
    ax = rng.normal(0.0, 1.0, (a.casts, 3))
    ax *= (rng.uniform(0.3, 1.5, a.casts) / np.linalg.norm(ax, axis=1))[:, None]
    casts["d"] = np.where((casts["tag"] == 1)[:, None], ax, 0.0)
    casts["p"] = csrc - 0.5 * casts["d"]
    casts["delta"] = dirn * rng.uniform(0.0, 6.0, (a.casts, 1))
    c = rng.uniform(lo, hi, (a.boxes, 3))
    half = rng.uniform(0.5, 2.0, (a.boxes, 1)) * np.ones((1, 3))  # one to four widths of a body of radius 0.5
    blo, bhi = (c - half).astype(np.float32), (c + half).astype(np.float32)

    def run(fn):
        fn()  # warm-up (allocations)
        b, r, wall = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            b.append(w.counter("query_build_ns") / 1e6)
            r.append(w.counter("query_run_ns") / 1e6)
        return dict(build_ms=float(np.median(b)), query_ms=float(np.median(r)), call_ms=float(np.median(wall))), out

    ray_t, hits = run(lambda: w.raycast(p, d, dt))
    sweep_t, shits = run(lambda: w.sweep(casts))
    box_t, (off, vals) = run(lambda: w.overlap_aabb(blo, bhi))
    print(json.dumps(dict(bodies=len(cen), ticks=a.ticks, rays=a.rays, ray_hits=int((hits["kind"] >= 0).sum()), raycast=ray_t,
                          casts=a.casts, sweep_hits=int((shits["kind"] >= 0).sum()), sweep=sweep_t,
                          boxes=a.boxes, overlap_results=int(off[-1]), overlap=box_t, large_bodies=w.counter("query_large_bodies"),
                          cells=w.counter("query_cells"))))
    ctx.close()


if __name__ == "__main__":
    main()
