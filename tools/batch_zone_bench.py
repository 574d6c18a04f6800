"""Times one iteration of a "who is near me" observation on a batch whose answer is consumed on the device, in the setting of
tools/batch_sensor_bench.py - K worlds of sphere_pile(8, 8, 8) after --ticks ticks, 64 zones a world, the library's work and torch's on
one stream, the paths rotating their order round by round, warm-up excluded, the median and the quartiles of --reps - two ways:
  (a) read_zones_dev of a rig set once - a box of half extent 1.5 sphere diameters about each of 64 bodies of every world, its own body
      left out, k = 8 - and the torch reduction of the counts (bodies in all zones of a world, the fullest zone of a world);
  (b) what a caller does without zones: gather_state of the same bodies, boxes by a torch expression, a copy to the host, overlap_boxes
      (mgf_batch_overlap_aabb_many: two launches, a prefix sum and a wait), the CSR lists copied back, the same reduction over the list
      lengths less the box's own body.
(b)'s centres are gather_state's x + delta, (a)'s are x without delta - where the colliders stand - so (b)'s boxes differ from (a)'s by
what the bodies move in a tick.  Before the timed rounds (b)'s steps behind the box expression - the copy to the host, overlap_boxes, the
lists - are therefore run once over the boxes (a) formed, and (a)'s records must equal the records restated from those lists byte for
byte; they must equal read_zones' too.  Run by hand; prints one JSON line per K."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgf_amd  # noqa: E402
from mgf_amd import scenes  # noqa: E402


def restated_records(off, bodies, own, k):
    """[n, 1 + k]: the length of list i less its own body, the first k of the rest, -1 behind them"""
    out = np.full((len(own), 1 + k), -1, np.int32)
    for i in range(len(own)):
        lst = bodies[off[i]:off[i + 1]].astype(np.int64)
        lst = lst[lst != own[i]]
        out[i, 0] = len(lst)
        out[i, 1:1 + min(k, len(lst))] = lst[:k]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[256], help="worlds")
    ap.add_argument("--zones", type=int, default=64, help="zones a world")
    ap.add_argument("--first", type=int, default=8, help="k: body indices a record holds")
    ap.add_argument("--half", type=float, default=1.5, help="half extent of a zone (a sphere's diameter is 1)")
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=31)
    a = ap.parse_args()
    ctx = mgf_amd.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    sc = scenes.sphere_pile(8, 8, 8)
    dt, iters, nb = float(sc["dt"]), sc["iters"], len(sc["comps"])
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
    except OSError:
        commit = ""
    with torch.cuda.stream(stream):
        for K in a.ks:
            b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
            b.step(dt, iters, a.ticks)
            per, n, k = a.zones, K * a.zones, a.first
            rng = np.random.default_rng(2)
            local = np.tile(rng.choice(nb, per, replace=False), K).astype(np.int32)
            world_np = np.repeat(np.arange(K, dtype=np.int32), per)
            d_body = torch.from_numpy((world_np * nb + local).astype(np.int32)).cuda()
            half = torch.full((n, 3), a.half, dtype=torch.float32, device="cuda")
            x = torch.empty((n, 3), dtype=torch.float32, device="cuda")
            out_a = torch.empty((n, 1 + k), dtype=torch.int32, device="cuda")
            box_a = torch.empty((n, 6), dtype=torch.float32, device="cuda")
            b.set_zones(world_np, local, (0.0, 0.0, 0.0), (a.half, a.half, a.half), True)
            result = {}

            def sync():
                stream.synchronize()

            def reduce(counts, key):
                c = counts.view(K, per)
                result[key] = (c.sum(dim=1), c.max(dim=1).values)

            def zones():
                b.read_zones_dev(out_a)
                reduce(out_a[:, 0], "zones")

            def assembled():
                b.gather_state(d_body, x=x)
                boxes = torch.cat([x, half], dim=1).cpu().numpy()          # (waits for the stream)
                off, bodies = b.overlap_boxes(world_np, boxes)
                d_off = torch.from_numpy(off).cuda()
                result["lists"] = torch.from_numpy(bodies.astype(np.int32)).cuda()
                reduce((d_off[1:] - d_off[:-1] - 1).to(torch.int32), "assembled")   # (a box about its own body holds it)

            sync()
            # once, unclocked: (a) against the host-memory form, and against (b)'s own steps run over the boxes (a) formed
            out_a.fill_(0x5A5A5A5A)
            b.read_zones_dev(out_a, boxes=box_a)
            sync()
            got = out_a.cpu().numpy()
            count, first = b.read_zones(k)
            off, bodies = b.overlap_boxes(world_np, box_a.cpu().numpy())
            equal = dict(read_zones=got.tobytes() == np.concatenate([count[:, None], first], axis=1).tobytes(),
                         overlap_boxes_lists=got.tobytes() == restated_records(off, bodies, local, k).tobytes())
            fns = (zones, assembled)
            t = {fn.__name__: [] for fn in fns}
            for rep in range(a.warmup + a.reps):
                for j in range(2):
                    fn = fns[(rep + j) % 2]
                    sync()
                    t0 = time.perf_counter()
                    fn()
                    sync()
                    if rep >= a.warmup:
                        t[fn.__name__].append(time.perf_counter() - t0)
            launches = {}
            for fn in fns:   # (unclocked)
                fn()
                launches[fn.__name__] = b.counter("query_launches")
            sync()
            med = {key: round(1e3 * float(np.median(v)), 4) for key, v in t.items()}
            quart = {key: [round(1e3 * float(q), 4) for q in np.percentile(v, [25, 75])] for key, v in t.items()}
            print(json.dumps(dict(K=K, bodies_per_world=nb, zones_per_world=per, k=k, half_extent=a.half, ticks=a.ticks, reps=a.reps,
                                  gpu=torch.cuda.get_device_name(0), commit=commit, median_ms=med, quartiles_ms=quart, query_launches=launches,
                                  bodies_in_zones=int(result["zones"][0].sum().item()), bodies_in_assembled_boxes=int(result["assembled"][0].sum().item()),
                                  fullest_zone=int(result["zones"][1].max().item()), equal=equal)), flush=True)
            del b
    stream.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
