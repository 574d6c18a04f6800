"""Times the observations of a batch (mgf_batch_read_body_contacts, mgf_batch_overlap_aabb_many) against the only other way to get them:
  (a) one read_body_contacts(-1) against K calls of mgf_batch_read_constraints plus the per-body fold on the host (numpy, vectorised:
      np.add.at - it gives the counts and, up to the order of the f32 sums, the impulses; the bit-exact fold is the call's);
  (b) 64 boxes per world in one call against K lone mgf_worlds holding the same state, one mgf_world_overlap_aabb_many call each.
K worlds of sphere_pile(8, 8, 8) after 60 ticks.  Wall clock around the synchronous calls, the two paths alternating in one process,
warm-up excluded, the median of --reps.  Run by hand; prints one JSON line per K.  The lone worlds get the batch's state one tick before
the end (write_state) and take the last tick themselves: a query sees the collider the last tick built, which write_state does not move."""
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


def host_fold(cons, n):
    """what a caller without the entry point does with one world's 96-byte records"""
    out = np.zeros(n, mgf_amd.BODY_CONTACTS_DTYPE)
    a, b = cons["a"], cons["b"]
    pair = b >= 0
    t = cons["normal"] * cons["normal_impulse"][:, None]
    np.add.at(out["n_contacts"], a, 1)
    np.add.at(out["n_contacts"], b[pair], 1)
    np.add.at(out["n_terrain"], a[~pair], 1)
    np.subtract.at(out["impulse"], a, t)
    np.add.at(out["impulse"], b[pair], t[pair])
    np.add.at(out["normal_impulse"], a, cons["normal_impulse"])
    np.add.at(out["normal_impulse"], b[pair], cons["normal_impulse"][pair])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 16, 256, 1024])
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--boxes", type=int, default=64, help="per world")
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
        box1 = np.empty((a.boxes, 6), np.float32)
        box1[:, :3] = cen[rng.integers(0, n, a.boxes)] + rng.normal(0, 0.5, (a.boxes, 3))
        box1[:, 3:] = rng.uniform(0.15, 1.5, (a.boxes, 1))
        world = np.repeat(np.arange(K, dtype=np.int32), a.boxes)
        boxes = np.tile(box1, (K, 1))
        lone = None
        if K <= a.lone_max:
            lone = [mgf_amd.World.from_scene(ctx, sc) for _ in range(K)]
            for k, w in enumerate(lone):
                w.write_state(**{f: before[f][k * n:(k + 1) * n] for f in STATE})
                w.step(dt, iters)
        t = dict(batch_contacts=[], loop_contacts=[], loop_contacts_read=[], batch_boxes=[], lone_boxes=[])
        run_ns = {}
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            got = b.body_contacts()
            t1 = time.perf_counter()
            run_ns["contacts"], launches_c = b.counter("query_run_ns"), b.counter("query_launches")
            t2 = time.perf_counter()
            lists = [b.constraints(k) for k in range(K)]
            t3 = time.perf_counter()
            folded = [host_fold(c, n) for c in lists]
            t4 = time.perf_counter()
            off, vals = b.overlap_boxes(world, boxes)
            t5 = time.perf_counter()
            run_ns["boxes"], launches_b = b.counter("query_run_ns"), b.counter("query_launches")
            row = dict(batch_contacts=t1 - t0, loop_contacts=t4 - t2, loop_contacts_read=t3 - t2, batch_boxes=t5 - t4)
            if lone is not None:
                t6 = time.perf_counter()
                lo = [w.overlap_boxes(box1) for w in lone]
                t7 = time.perf_counter()
                row["lone_boxes"] = t7 - t6
            if rep >= a.warmup:
                for key, v in row.items():
                    t[key].append(v)
        med = {k: float(np.median(v)) for k, v in t.items() if v}
        folded = np.concatenate(folded)
        records = int(sum(len(c) for c in lists))
        out = dict(K=K, bodies_per_world=n, ticks=a.ticks, boxes_per_world=a.boxes, records=records, record_bytes=96 * records, answer_bytes=24 * len(got),
                   batch_contacts_ms=1e3 * med["batch_contacts"], loop_contacts_ms=1e3 * med["loop_contacts"],
                   loop_contacts_read_ms=1e3 * med["loop_contacts_read"], contacts_speedup=med["loop_contacts"] / med["batch_contacts"],
                   batch_contacts_run_ns=run_ns["contacts"], query_launches_contacts=launches_c,
                   counts_equal=bool(np.array_equal(got["n_contacts"], folded["n_contacts"]) and np.array_equal(got["n_terrain"], folded["n_terrain"])),
                   impulse_max_abs_diff=float(np.max(np.abs(got["impulse"] - folded["impulse"]), initial=0.0)),
                   batch_boxes_ms=1e3 * med["batch_boxes"], batch_boxes_run_ns=run_ns["boxes"], query_launches_boxes=launches_b, box_hits=int(len(vals)))
        if lone is not None:
            same = bool(np.array_equal(np.concatenate([v for _, v in lo]), vals)
                        and np.array_equal(np.concatenate([[0]] + [o[1:] + k * int(lo[0][0][-1]) for k, (o, _) in enumerate(lo)]), off))
            out.update(lone_boxes_ms=1e3 * med["lone_boxes"], boxes_speedup=med["lone_boxes"] / med["batch_boxes"], box_answers_equal=same)
        print(json.dumps(out), flush=True)
        del b, lone
    ctx.close()


if __name__ == "__main__":
    main()
