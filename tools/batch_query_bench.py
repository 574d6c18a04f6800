"""Times the queries of a batch (mgf_batch_raycast_many / mgf_batch_sweep_many) against the only other way to ask K small worlds: K lone
mgf_worlds holding the same state, one mgf_world_raycast_many / mgf_world_sweep_many call each.  K worlds of sphere_pile(8, 8, 8) after 60
ticks, 64 rays and 16 casts per world.  Wall clock around the synchronous calls, the two paths alternating in one process, warm-up
excluded, the median of --reps.  Run by hand; prints one JSON line per K:
  wall time of the batch call and of the loop of lone calls (K <= --lone-max), the batch's "query_run_ns" and "query_launches", and the exact
  ray-body tests per second of the batch call (the tests that pass the bounding-sphere reject, counted on the host with the reject's formula).
The lone worlds get the batch's state one tick before the end (write_state) and take the last tick themselves: a query sees the collider
the last tick built, which write_state does not move."""
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


def exact_ray_tests(p, d, centres, radius):
    """rays x bodies that pass k_batch_query_ray's bounding-sphere reject (bq_ray_far, spheres), in f32"""
    f = np.float32
    w = centres[None, :, :].astype(f) - p[:, None, :].astype(f)
    dd = np.einsum("ij,ij->i", d, d).astype(f)
    s = np.maximum(np.einsum("ijk,ik->ij", w, d).astype(f) / dd[:, None], f(0))
    e = w - d[:, None, :] * s[:, :, None]
    lim = f(radius) * f(1.01) + f(1e-3)
    return int(np.sum(~(np.einsum("ijk,ijk->ij", e, e) > lim * lim + f(1e-4) * np.einsum("ijk,ijk->ij", w, w))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 16, 256, 1024])
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--rays", type=int, default=64, help="per world")
    ap.add_argument("--casts", type=int, default=16, help="per world")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lone-max", type=int, default=1024)
    a = ap.parse_args()
    ctx = mgf_amd.Context(0)
    sc = scenes.sphere_pile(8, 8, 8)
    dt, iters, n = float(sc["dt"]), sc["iters"], len(sc["comps"])
    for K in a.ks:
        b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
        b.step(dt, iters, a.ticks - 1)
        before = b.state() if K <= a.lone_max else None
        b.step(dt, iters, 1)
        cen = b.colliders(0)["p"]
        rng = np.random.default_rng(1)
        tgt = cen[rng.integers(0, n, a.rays)] + rng.normal(0, 0.3, (a.rays, 3))
        p1 = (tgt + rng.normal(0, 2.0, (a.rays, 3)) + (0.0, 14.0, 0.0)).astype(np.float32)
        d1 = (tgt - p1).astype(np.float32)
        c1 = np.zeros(a.casts, mgf_amd.MOVING_DTYPE)
        c1["tag"] = np.arange(a.casts) % 2
        c1["r"] = 0.3
        c1["d"][c1["tag"] == 1] = (0.6, 0.2, 0.0)
        src = cen[rng.integers(0, n, a.casts)] + (0.0, 10.0, 0.0) + rng.normal(0, 1.0, (a.casts, 3))
        c1["p"] = src
        c1["delta"] = cen[rng.integers(0, n, a.casts)] - src
        world_r = np.repeat(np.arange(K, dtype=np.int32), a.rays)
        world_c = np.repeat(np.arange(K, dtype=np.int32), a.casts)
        p, d, casts = np.tile(p1, (K, 1)), np.tile(d1, (K, 1)), np.tile(c1, K)
        lone = None
        if K <= a.lone_max:
            lone = [mgf_amd.World.from_scene(ctx, sc) for _ in range(K)]
            for k, w in enumerate(lone):
                w.write_state(**{f: before[f][k * n:(k + 1) * n] for f in STATE})
                w.step(dt, iters)
        t = dict(batch_rays=[], batch_casts=[], lone_rays=[], lone_casts=[])
        run_ns = {}
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            hr = b.raycast(world_r, p, d)
            t1 = time.perf_counter()
            run_ns["rays"], launches_r = b.counter("query_run_ns"), b.counter("query_launches")
            t2 = time.perf_counter()
            hs = b.sweep(world_c, casts)
            t3 = time.perf_counter()
            run_ns["casts"], launches_s = b.counter("query_run_ns"), b.counter("query_launches")
            row = [t1 - t0, t3 - t2]
            if lone is not None:
                t4 = time.perf_counter()
                lr = [w.raycast(p1, d1) for w in lone]
                t5 = time.perf_counter()
                ls = [w.sweep(c1) for w in lone]
                t6 = time.perf_counter()
                row += [t5 - t4, t6 - t5]
            if rep >= a.warmup:
                for key, v in zip(t, row):
                    t[key].append(v)
        med = {k: float(np.median(v)) for k, v in t.items() if v}
        tests = exact_ray_tests(p1, d1, cen, 0.5) * K
        out = dict(K=K, bodies_per_world=n, ticks=a.ticks, rays_per_world=a.rays, casts_per_world=a.casts,
                   batch_rays_ms=1e3 * med["batch_rays"], batch_casts_ms=1e3 * med["batch_casts"], batch_rays_run_ns=run_ns["rays"],
                   batch_casts_run_ns=run_ns["casts"], query_launches_rays=launches_r, query_launches_casts=launches_s,
                   ray_body_hits=int(np.sum(hr["kind"] == 0)), cast_body_hits=int(np.sum(hs["kind"] == 0)),
                   exact_ray_body_tests=tests, exact_ray_body_tests_per_s=tests / med["batch_rays"])
        if lone is not None:
            same = bool(np.concatenate(lr).tobytes() == hr.tobytes() and np.concatenate(ls).tobytes() == hs.tobytes())
            out.update(lone_rays_ms=1e3 * med["lone_rays"], lone_casts_ms=1e3 * med["lone_casts"], rays_speedup=med["lone_rays"] / med["batch_rays"],
                       casts_speedup=med["lone_casts"] / med["batch_casts"], answers_equal=same)
        print(json.dumps(out), flush=True)
        del b, lone
    ctx.close()


if __name__ == "__main__":
    main()
