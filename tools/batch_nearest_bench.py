"""Times one iteration of a "my k nearest neighbours" observation on a batch whose answer is consumed on the device, in the setting of
tools/batch_zone_bench.py - K worlds of sphere_pile(8, 8, 8) after --ticks ticks, 64 zones a world, a box of half extent --half about
each of 64 bodies of every world, its own body left out, k = 8, the library's work and torch's on one stream, the paths rotating their
order round by round, warm-up excluded, the median and the quartiles of --reps - two ways:
  (a) read_zones_nearest_dev of a rig set once, with the distances, and a torch reduction of the result (per world the bodies in all
      zones and the mean squared distance of the nearest neighbours that exist);
  (b) what a caller assembles without it: read_zones_dev with a k large enough for the fullest zone (found once, unclocked), gather_state
      of every body, the listed bodies' positions by torch indexing, squared distances from the zone body's position, +inf where the
      record holds -1, torch.topk of the k smallest, the same reduction.
(b)'s positions are gather_state's x + delta and its sums are torch's, (a)'s centres are the colliders' and its sums the header's: the
two agree to rounding and to what the bodies move in a tick, not to the bit, so the tool reports the largest difference of the reduced
figures and holds (a) to its own definition instead: before the timed rounds (a)'s records and distances must equal the host-memory
form's byte for byte, and the restatement over overlap_boxes' lists and colliders().  Run by hand; prints one JSON line per K."""
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


def restated(off, bodies, own, world, centres, boxes, k):
    """([n, 1 + k] int32, [n, k] float32): per box the length of its list less its own body, the rest in ascending (d2, index), -1 / +inf
    behind them; centres[w]: the tight-box centres of world w, rows by body index"""
    f32 = np.float32
    out, dd = np.full((len(own), 1 + k), -1, np.int32), np.full((len(own), k), np.inf, f32)
    for i in range(len(own)):
        lst = bodies[off[i]:off[i + 1]].astype(np.int64)
        lst = lst[lst != own[i]]
        e = centres[world[i]][lst] - boxes[i, :3]
        sq = e * e
        d2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
        by = np.argsort(d2, kind="stable")[:k]
        out[i, 0] = len(lst)
        out[i, 1:1 + len(by)], dd[i, :len(by)] = lst[by], d2[by]
    return out, dd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[256], help="worlds")
    ap.add_argument("--zones", type=int, default=64, help="zones a world")
    ap.add_argument("--nearest", type=int, default=8, help="k: the nearest bodies a record holds")
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
            per, n, k = a.zones, K * a.zones, a.nearest
            rng = np.random.default_rng(2)
            local = np.tile(rng.choice(nb, per, replace=False), K).astype(np.int32)
            world_np = np.repeat(np.arange(K, dtype=np.int32), per)
            d_own = torch.from_numpy((world_np.astype(np.int64) * nb + local)).cuda()
            d_base = torch.from_numpy(world_np.astype(np.int64) * nb).cuda()[:, None]
            b.set_zones(world_np, local, (0.0, 0.0, 0.0), (a.half, a.half, a.half), True)
            out_a = torch.empty((n, 1 + k), dtype=torch.int32, device="cuda")
            d2_a = torch.empty((n, k), dtype=torch.float32, device="cuda")
            box_a = torch.empty((n, 6), dtype=torch.float32, device="cuda")
            x_all = torch.empty((K * nb, 3), dtype=torch.float32, device="cuda")
            inf = torch.tensor(float("inf"), dtype=torch.float32, device="cuda")
            result = {}

            def sync():
                stream.synchronize()

            def reduce(count, d2, key):
                real = torch.isfinite(d2)
                mean = torch.where(real, d2, torch.zeros_like(d2)).view(K, -1).sum(dim=1) / real.view(K, -1).sum(dim=1).clamp(min=1)
                result[key] = (count.view(K, per).sum(dim=1), mean)

            # once, unclocked: the fullest zone sizes (b)'s records; (a) against the host-memory form and against its definition
            sync()
            out_a.fill_(0x5A5A5A5A)
            d2_a.view(torch.int32).fill_(0x5A5A5A5A)
            b.read_zones_nearest_dev(out_a, dist2=d2_a, boxes=box_a)
            sync()
            got, got_d = out_a.cpu().numpy(), d2_a.cpu().numpy()
            count, near, hd = b.read_zones_nearest(k, dist2=True)
            boxes_np = box_a.cpu().numpy()
            off, bodies = b.overlap_boxes(world_np, boxes_np)
            cols = b.colliders()
            cen = cols["p"].astype(np.float32).reshape(K, nb, 3)       # (spheres: the tight box's centre is the collider's)
            want, want_d = restated(off, bodies, local, world_np, cen, boxes_np, k)
            equal = dict(host_form=got.tobytes() == np.concatenate([count[:, None], near], axis=1).tobytes() and got_d.tobytes() == hd.tobytes(),
                         restated=got.tobytes() == want.tobytes() and got_d.tobytes() == want_d.tobytes())
            kb = int(count.max())
            out_b = torch.empty((n, 1 + kb), dtype=torch.int32, device="cuda")

            def nearest():
                b.read_zones_nearest_dev(out_a, dist2=d2_a)
                reduce(out_a[:, 0], d2_a, "nearest")

            def assembled():
                b.read_zones_dev(out_b)
                b.gather_state(None, x=x_all)
                idx = out_b[:, 1:].to(torch.int64)
                listed = idx >= 0
                pos = x_all[(idx.clamp(min=0) + d_base).view(-1)].view(n, kb, 3)
                e = pos - x_all[d_own][:, None, :]
                d2 = torch.where(listed, (e * e).sum(dim=2), inf)
                best, at = torch.topk(d2, k, dim=1, largest=False)
                result["assembled_bodies"] = torch.where(torch.isfinite(best), torch.gather(idx, 1, at), torch.full_like(at, -1))
                reduce(out_b[:, 0], best, "assembled")

            fns = (nearest, assembled)
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
            same_bodies = float((result["assembled_bodies"] == out_a[:, 1:].to(torch.int64)).float().mean().item())
            med = {key: round(1e3 * float(np.median(v)), 4) for key, v in t.items()}
            quart = {key: [round(1e3 * float(q), 4) for q in np.percentile(v, [25, 75])] for key, v in t.items()}
            print(json.dumps(dict(K=K, bodies_per_world=nb, zones_per_world=per, k=k, k_assembled=kb, half_extent=a.half, ticks=a.ticks, reps=a.reps,
                                  gpu=torch.cuda.get_device_name(0), commit=commit, median_ms=med, quartiles_ms=quart, query_launches=launches,
                                  bodies_in_zones=int(result["nearest"][0].sum().item()), bodies_in_assembled_zones=int(result["assembled"][0].sum().item()),
                                  mean_d2_max_difference=float((result["nearest"][1] - result["assembled"][1]).abs().max().item()),
                                  assembled_names_the_same_body=round(same_bodies, 4), equal=equal)), flush=True)
            del b
    stream.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
