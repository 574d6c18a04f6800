"""Times K small worlds of bodies of up to four components stepped as one batch (mgf_batch_step, the part-aware tick of k_batch_parts.h)
against the same K scenes as K lone mgf_worlds on one context stepped in turn, for K worlds of dumbbell_field(4, 3, 4, n_plain=16) - 64
bodies of one and two parts - and of jack_field(4, 2, 4) - 32 bodies of four parts - from tick 0, in the style of tools/batch_bench.py:
wall clock around synchronous calls (both paths drain the context's stream before they return), warm-up excluded, both paths on the same
build in the same run, the windows of the two alternating.  Run by hand; prints one JSON line per (scene, K): ms per tick of the batch
and of the loop of lone worlds as quartiles (q1, median, q3) over --reps windows each, world-ticks per second, the constraints of a tick."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgf_amd  # noqa: E402
from mgf_amd import scenes  # noqa: E402

SCENES = {"dumbbell_field": lambda: scenes.dumbbell_field(4, 3, 4, n_plain=16), "jack_field": lambda: scenes.jack_field(4, 2, 4)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def quartiles(t, per):
    q = np.percentile(np.asarray(t) / per * 1e3, [25, 50, 75])
    return [float(v) for v in q]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--scenes", nargs="+", default=list(SCENES), choices=list(SCENES))
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--window", type=int, default=20, help="ticks per timed window of the batch")
    ap.add_argument("--lone-window", type=int, default=4, help="ticks per timed window of the loop of lone worlds")
    ap.add_argument("--reps", type=int, default=7, help="windows per path (at least five)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    ctx = mgf_amd.Context(0)
    for name in a.scenes:
        sc = SCENES[name]()
        dt, iters = float(sc["dt"]), sc["iters"]
        n = len(sc["comps"]) + len(sc["compound"]["offsets"]) - 1
        for K in a.ks:
            b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
            lone = [mgf_amd.World.from_scene(ctx, sc) for _ in range(K)]
            b.step(dt, iters, a.warmup)
            for w in lone:
                for _ in range(a.warmup):
                    w.step(dt, iters)
            cons, t_batch, t_lone = [], [], []

            def batch_window():
                st = b.step(dt, iters, a.window)
                cons.append(sum(s.n_constraints for s in st) / a.window)

            def lone_window():
                for _ in range(a.lone_window):
                    for w in lone:
                        w.step(dt, iters)
            for _ in range(a.reps):  # the two paths alternate: whatever else the host does meets both
                t_batch.append(timed(batch_window))
                t_lone.append(timed(lone_window))
            qb, ql = quartiles(t_batch, a.window), quartiles(t_lone, a.lone_window)
            print(json.dumps(dict(scene=name, bodies_per_world=n, K=K, iters=iters, reps=a.reps, batch_ms_per_tick_q1_med_q3=qb, lone_ms_per_tick_q1_med_q3=ql,
                                  batch_world_ticks_per_s=K / (qb[1] * 1e-3), lone_world_ticks_per_s=K / (ql[1] * 1e-3), batch_speedup=ql[1] / qb[1],
                                  constraints_per_tick=float(np.median(cons)), launches_per_tick=b.counter("launches_per_tick"),
                                  capacity_retries=b.counter("capacity_retries"))), flush=True)
            del b, lone
    ctx.close()


if __name__ == "__main__":
    main()
