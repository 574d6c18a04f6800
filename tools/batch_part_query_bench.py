"""Times the part-aware queries of a batch (mgf_batch_set_option "part_queries"; k_batch_part_query.h) on K worlds of
tools/batch_parts_bench.py's dumbbell scene - dumbbell_field(4, 3, 4, n_plain=16): 64 bodies, 48 of them of two parts - as added (tick
0: every path then holds the same shapes at the same places), --per rays, casts and box zones a world, three ways:
  (a) one raycast / sweep / read_zones_dev call on the batch with the option on (the kernels k_batch_pq_*);
  (b) the same queries as K lone-world calls in turn (World.raycast / sweep / overlap_boxes), the condition being (a) < (b) - printed
      per call as "batch_below_lone" and for all three as "condition_batch_below_lone_loop";
  (c) the same calls on a batch whose parts were added as ordinary bodies - 112 a world - which runs the existing kernels and shows
      what the part path costs: (a) / (c) is reported, no ratio is fixed in advance.
Before the timed rounds (a)'s answers are compared with (b)'s: equal bytes, the zones' counts and lists.  Wall clock around calls that have waited for the device
(read_zones_dev: a device-wide wait behind it), warm-up excluded, the three paths rotating their order round by round, the median and
the quartiles of --reps.  Run by hand; prints one JSON line per K."""
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


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def quartiles(t):
    return [float(v) for v in np.percentile(np.asarray(t) * 1e3, [25, 50, 75])]


def queries(sc, per, seed):
    """rays from above aimed at the parts, casts (half spheres, half capsules) from beside them, boxes around them: one world's"""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([sc["comps"], sc["compound"]["comps"]])
    cen = rows["p"].astype(np.float64) + 0.5 * rows["d"] * (rows["tag"] == 1)[:, None]
    tgt = cen[rng.integers(0, len(cen), per)] + rng.normal(0, 0.3, (per, 3))
    p = tgt + rng.normal(0, 1.0, (per, 3)) + np.array([0.0, 8.0, 0.0])
    casts = np.zeros(per, mgf_amd.MOVING_DTYPE)
    src = cen[rng.integers(0, len(cen), per)] + rng.normal(0, 0.3, (per, 3)) + np.array([0.0, 1.5, 0.0])
    to = cen[rng.integers(0, len(cen), per)] - src
    casts["tag"] = np.arange(per) % 2
    casts["r"] = rng.uniform(0.2, 0.6, per)
    ax = rng.normal(0, 1, (per, 3))
    ax *= (rng.uniform(0.3, 1.5, per) / np.linalg.norm(ax, axis=1))[:, None]
    casts["d"] = np.where((casts["tag"] == 1)[:, None], ax, 0.0)
    casts["p"] = src - 0.5 * casts["d"]
    casts["delta"] = to / np.maximum(np.linalg.norm(to, axis=1, keepdims=True), 1e-9) * rng.uniform(0.0, 5.0, (per, 1))
    boxes = np.concatenate([cen[rng.integers(0, len(cen), per)], np.full((per, 3), 1.0)], axis=1).astype(np.float32)
    return p.astype(np.float32), (tgt - p).astype(np.float32), casts, boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[256])
    ap.add_argument("--per", type=int, default=64, help="rays, casts and zones a world")
    ap.add_argument("--k", type=int, default=8, help="bodies a zone's record holds")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=31)
    a = ap.parse_args()
    ctx = mgf_amd.Context(0)
    sc = scenes.dumbbell_field(4, 3, 4, n_plain=16)
    cb = sc["compound"]
    n_parts = len(cb["comps"])
    per_part = np.repeat(np.arange(len(cb["offsets"]) - 1), np.diff(cb["offsets"]))
    flat = dict(sc, compound=None, v0=None, comps=np.concatenate([sc["comps"], cb["comps"]]), mass=np.concatenate([sc["mass"], cb["comp_mass"]]),
                restitution=np.concatenate([sc["restitution"], cb["restitution"][per_part]]), friction=np.concatenate([sc["friction"], cb["friction"][per_part]]),
                force=np.concatenate([sc["force"], cb["force"][per_part]]))
    assert len(flat["comps"]) == len(sc["comps"]) + n_parts
    p1, d1, c1, z1 = queries(sc, a.per, 7)
    for K in a.ks:
        n = K * a.per
        world = np.repeat(np.arange(K, dtype=np.int32), a.per)
        p, d, casts, boxes = np.tile(p1, (K, 1)), np.tile(d1, (K, 1)), np.tile(c1, K), np.tile(z1, (K, 1))
        on = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
        on.set_option("part_queries", 1)
        plain = mgf_amd.WorldBatch.from_scenes(ctx, [flat] * K)
        lone = [mgf_amd.World.from_scene(ctx, sc) for _ in range(K)]
        out = {b: torch.zeros((n, 1 + a.k), dtype=torch.int32, device="cuda") for b in (on, plain)}
        torch.cuda.synchronize()
        for b in (on, plain):
            b.set_zones(world, -1, boxes[:, :3], boxes[:, 3:])

        def zones(b):
            b.read_zones_dev(out[b])
            torch.cuda.synchronize()
        # (a) against (b): equal bytes
        ra, sa = on.raycast(world, p, d), on.sweep(world, casts)
        zones(on)
        za = out[on].cpu().numpy()
        for k in range(K):
            s = slice(k * a.per, (k + 1) * a.per)
            assert ra[s].tobytes() == lone[k].raycast(p1, d1).tobytes() and sa[s].tobytes() == lone[k].sweep(c1).tobytes(), k
            off, vals = lone[k].overlap_boxes(z1)
            assert np.array_equal(za[s, 0], np.diff(off).astype(np.int32)), k
            for i in range(a.per):   # the record: the first k of the lone world's list, then -1
                li = vals[off[i]:off[i + 1]][:a.k].astype(np.int32)
                assert np.array_equal(za[s][i, 1:1 + len(li)], li) and np.all(za[s][i, 1 + len(li):] == -1), (k, i)
        paths = {
            "ray": dict(on=lambda: on.raycast(world, p, d), lone=lambda: [w.raycast(p1, d1) for w in lone], plain=lambda: plain.raycast(world, p, d)),
            "sweep": dict(on=lambda: on.sweep(world, casts), lone=lambda: [w.sweep(c1) for w in lone], plain=lambda: plain.sweep(world, casts)),
            "zones": dict(on=lambda: zones(on), lone=lambda: [w.overlap_boxes(z1) for w in lone], plain=lambda: zones(plain)),
        }
        res = dict(K=K, per_world=a.per, bodies_per_world=len(lone[0]), plain_bodies_per_world=len(flat["comps"]), reps=a.reps, zone_k=a.k,
                   hits_on_parts=int(np.sum((ra["kind"] == 0) & (ra["index"] >= len(sc["comps"])))), ray_hits_part_above_0=int(np.sum(ra["part"] > 0)))
        for name, three in paths.items():
            t = {w: [] for w in three}
            order = list(three)
            for r in range(a.warmup + a.reps):
                for w in order[r % 3:] + order[:r % 3]:   # the paths rotate their order round by round
                    dtm = timed(three[w])
                    if r >= a.warmup:
                        t[w].append(dtm)
            q = {w: quartiles(v) for w, v in t.items()}
            res[name] = dict(batch_on_ms_q1_med_q3=q["on"], lone_loop_ms_q1_med_q3=q["lone"], batch_plain_ms_q1_med_q3=q["plain"],
                             lone_over_on=q["lone"][1] / q["on"][1], on_over_plain=q["on"][1] / q["plain"][1],
                             batch_below_lone=bool(q["on"][1] < q["lone"][1]))
        res["condition_batch_below_lone_loop"] = all(res[name]["batch_below_lone"] for name in paths)   # the standing condition of batch features
        print(json.dumps(res), flush=True)
        del on, plain, lone
    ctx.close()


if __name__ == "__main__":
    main()
