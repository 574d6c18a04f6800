"""Times the device-pointer calls of a batch against the host-memory calls, for a caller whose records are CUDA tensors:
  (a) set_forces_dev + apply_impulses_dev on --records records held as CUDA tensors, against .cpu() of those tensors and then
      set_forces + apply_impulses;
  (b) gather_state of all bodies into CUDA tensors, against a whole-batch get and torch.from_numpy(...).cuda() of its fields;
  (c) copy_worlds_where with a CUDA mask that selects --copies of K pairs, against .cpu() of the mask and copy_worlds of those pairs.
K worlds of sphere_pile(8, 8, 8) after --ticks ticks (the snapshot after half of them), the setting of tools/batch_drive_bench.py.  Wall
clock from the call to a completed torch.cuda.synchronize(), the paths alternating in one process, every interval with a clock of its
own, the two paths of a comparison taking turns in going first, warm-up excluded, the median and the quartiles of --reps (and the medians
by place in the round).  Before the timed rounds each new path is checked once against its comparator.  Run by hand; prints one JSON line
per K."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgf_amd  # noqa: E402
from mgf_amd import scenes  # noqa: E402

GATHER = ("x", "v", "omega", "force", "torque")
GET = ("x", "linear", "angular", "force", "torque")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[256])
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--records", type=int, default=4096)
    ap.add_argument("--copies", type=int, default=64, help="pairs the mask selects")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=31)
    a = ap.parse_args()
    ctx = mgf_amd.Context(0)
    sc = scenes.sphere_pile(8, 8, 8)
    dt, iters, n = float(sc["dt"]), sc["iters"], len(sc["comps"])
    sync = torch.cuda.synchronize
    for K in a.ks:
        b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
        snap = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
        snap.step(dt, iters, a.ticks // 2)
        b.step(dt, iters, a.ticks)
        total = len(b)
        rng = np.random.default_rng(1)
        flat = rng.choice(total, min(a.records, total), replace=False).astype(np.int32)
        world_np, body_np = (flat // n).astype(np.int32), (flat % n).astype(np.int32)
        R = len(flat)
        d_flat, d_world, d_body = (torch.from_numpy(x).cuda() for x in (flat, world_np, body_np))
        d_rows = [torch.from_numpy(rng.uniform(-1, 1, (R, 3)).astype(np.float32)).cuda() for _ in range(4)]   # force, torque, linear, angular
        all_world, all_body = np.repeat(np.arange(K, dtype=np.int32), n), np.tile(np.arange(n, dtype=np.int32), K)
        out = {k: torch.empty((total, 3), dtype=torch.float32, device="cuda") for k in GATHER}
        pairs = np.arange(K, dtype=np.int32)
        mask_np = np.zeros(K, np.int32)
        mask_np[rng.choice(K, min(a.copies, K), replace=False)] = 1
        d_mask = torch.from_numpy(mask_np).cuda()
        sync()
        # once, unclocked: the new paths give what their comparators give
        b.gather_state(None, **out)
        sync()
        got = b.get(all_world, all_body)
        gather_equal = all(out[k].cpu().numpy().tobytes() == got[g].tobytes() for k, g in zip(GATHER, GET))
        b.copy_worlds_where(pairs, snap, pairs, d_mask)
        sync()
        sel = np.flatnonzero(mask_np)
        copy_equal = all(b.state(int(k))["x"].tobytes() == snap.state(int(k))["x"].tobytes() and
                         b.constraints(int(k)).tobytes() == snap.constraints(int(k)).tobytes() for k in sel[:4])
        t = dict(drive_dev=[], drive_host=[], gather_dev=[], gather_host=[], copy_dev=[], copy_host=[])
        by_place = {k: ([], []) for k in t}   # the same intervals by whether the path went first or second in its round
        launches = {}
        host_out = None

        def drive_dev():
            b.set_forces_dev(d_flat, d_rows[0], d_rows[1])
            b.apply_impulses_dev(d_flat, d_rows[2], d_rows[3])

        def drive_host():
            w, bd = d_world.cpu().numpy(), d_body.cpu().numpy()
            f, tq, li, an = (r.cpu().numpy() for r in d_rows)
            b.set_forces(w, bd, f, tq)
            b.apply_impulses(w, bd, li, an)

        def gather_dev():
            b.gather_state(None, **out)

        def gather_host():
            nonlocal host_out
            got = b.get(all_world, all_body)
            host_out = {k: torch.from_numpy(np.ascontiguousarray(got[g])).cuda() for k, g in zip(GATHER, GET)}

        def copy_dev():
            b.copy_worlds_where(pairs, snap, pairs, d_mask)

        def copy_host():
            which = np.flatnonzero(d_mask.cpu().numpy()).astype(np.int32)
            b.copy_worlds(which, snap, which)

        def clocked(fn):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            return time.perf_counter() - t0
        for rep in range(a.warmup + a.reps):
            # the two paths of a comparison take turns in going first: whoever follows the other finds the same rows warm in the caches
            for new, old in ((drive_dev, drive_host), (gather_dev, gather_host), (copy_dev, copy_host)):
                for place, fn in enumerate((new, old) if rep % 2 == 0 else (old, new)):
                    dt_s = clocked(fn)
                    if rep >= a.warmup:
                        t[fn.__name__].append(dt_s)
                        by_place[fn.__name__][place].append(dt_s)
        for key, fn in (("setters_dev", drive_dev), ("gather_dev", gather_dev), ("copy_dev", copy_dev)):   # (unclocked)
            fn()
            launches[key] = b.counter("drive_launches")
        sync()
        del host_out
        med = {k: round(1e3 * float(np.median(v)), 4) for k, v in t.items()}
        quart = {k: [round(1e3 * float(q), 4) for q in np.percentile(v, [25, 75])] for k, v in t.items()}
        print(json.dumps(dict(K=K, bodies_per_world=n, ticks=a.ticks, records=R, pairs=K, copies=int(mask_np.sum()), reps=a.reps, median_ms=med, quartiles_ms=quart,
                              median_ms_first_second={k: [round(1e3 * float(np.median(x)), 4) for x in v] for k, v in by_place.items()},
                              drive_dev_below_host=med["drive_dev"] < med["drive_host"], gather_dev_below_host=med["gather_dev"] < med["gather_host"],
                              copy_dev_below_host=med["copy_dev"] < med["copy_host"], drive_launches=launches,
                              pair_table_uploads=b.counter("pair_table_uploads"), device_skipped=b.counter("device_skipped"),
                              gather_equal=bool(gather_equal), copied_equal=bool(copy_equal))), flush=True)
        del b, snap
    ctx.close()


if __name__ == "__main__":
    main()
