"""Times one iteration of a feeler loop on a batch whose hits are consumed on the device, in the setting of
tools/batch_sensor_bench.py - K worlds of sphere_pile(8, 8, 8) after --ticks ticks, 64 feelers a world (spheres of radius 0.1 at the
centre of their body, swept one body length along the body's own -y, their own body ignored), mask QUERY_ALL, the library's work and
torch's on one stream, the paths rotating their order round by round, warm-up excluded, the median and the quartiles of --reps - two
ways:
  (a) cast_feelers_dev of a rig set once, and the torch reduction of the hits (hits per world, the earliest t per world, the mean
      normal's y per world);
  (b) the assembly a caller needs without the rig: gather_state of the feeler bodies (x and q), a torch expression that turns p, d
      and delta by q and writes the casts, sweep_dev with the fixed layout and the same ignore values, the same reduction.  ((b)'s x
      is x + delta and its rotate is torch's arithmetic: its casts are close to (a)'s, not equal to the bit.)
Before the timed rounds the hits of (a) are compared with cast_feelers and with sweep of casts made on the host from state(): equal
bytes.  Run by hand; prints one JSON line per K."""
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


def np_rotate(q, r):
    """Rotation::rotate_vector in f32, operation by operation"""
    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    s, v = q[:, 0:1], q[:, 1:4]
    return cross(v, cross(v, r) + r * s) * np.float32(2.0) + r


def torch_rotate(q, r):
    s, v = q[:, 0:1], q[:, 1:4]
    return torch.linalg.cross(v, torch.linalg.cross(v, r) + r * s) * 2.0 + r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[256])
    ap.add_argument("--feelers", type=int, default=64, help="feelers a world")
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
            per, n = a.feelers, K * a.feelers
            rng = np.random.default_rng(2)
            local = np.tile(rng.choice(nb, per, replace=False), K).astype(np.int32)
            world_np = np.repeat(np.arange(K, dtype=np.int32), per)
            body_np = (world_np * nb + local).astype(np.int32)
            p_np, d_np = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
            delta_np = np.tile(np.float32([0.0, -1.0, 0.0]), (n, 1))          # one body length (the spheres' diameter)
            radius = np.float32(0.1)
            d_body = torch.from_numpy(body_np).cuda()
            d_local = torch.from_numpy(local).cuda()
            d_p, d_d, d_delta = (torch.from_numpy(v).cuda() for v in (p_np, d_np, delta_np))
            tag_r = torch.zeros((n, 1), dtype=torch.float32, device="cuda")    # (the bits of tag 0)
            rad = torch.full((n, 1), float(radius), dtype=torch.float32, device="cuda")
            x = torch.empty((n, 3), dtype=torch.float32, device="cuda")
            q = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            out_a = torch.empty((n, 13), dtype=torch.int32, device="cuda")
            out_b = torch.empty((n, 13), dtype=torch.int32, device="cuda")
            b.set_feelers(world_np, local, tag=0, p=p_np, d=d_np, r=radius, delta=delta_np, ignore_self=True)
            result = {}

            def sync():
                stream.synchronize()

            def reduce(hits, key):
                h = hits.view(K, per, 13)
                met = h[..., 0] >= 0
                t = torch.where(met, h[..., 12].view(torch.float32), torch.full((), float("inf"), device="cuda"))
                ny = torch.where(met, h[..., 10].view(torch.float32), torch.zeros((), device="cuda"))
                result[key] = (met.sum(dim=1), t.min(dim=1).values, ny.mean(dim=1))

            def feelers():
                b.cast_feelers_dev(out_a)
                reduce(out_a, "feelers")

            def assembled():
                b.gather_state(d_body, x=x, q=q)
                casts = torch.cat([tag_r, x + torch_rotate(q, d_p), torch_rotate(q, d_d), rad, torch_rotate(q, d_delta)], dim=1)
                b.sweep_dev(None, casts, out_b, ignore=d_local)
                reduce(out_b, "assembled")

            sync()
            # once, unclocked: (a) against the host-memory form and against sweep of casts made on the host from state()
            out_a.fill_(0x5A5A5A5A)
            feelers()
            sync()
            got = out_a.cpu().numpy().tobytes()
            st = b.state()
            c = np.zeros(n, mgf_amd.MOVING_DTYPE)
            c["r"], c["p"], c["d"] = radius, st["x"][body_np] + np_rotate(st["q"][body_np], p_np), np_rotate(st["q"][body_np], d_np)
            c["delta"] = np_rotate(st["q"][body_np], delta_np)
            equal = dict(cast_feelers=got == b.cast_feelers().tobytes(), sweep_from_state=got == b.sweep(world_np, c, None, ignore=local).tobytes())
            fns = (feelers, assembled)
            t = {fn.__name__: [] for fn in fns}
            for rep in range(a.warmup + a.reps):
                for k in range(2):
                    fn = fns[(rep + k) % 2]
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
            med = {k: round(1e3 * float(np.median(v)), 4) for k, v in t.items()}
            quart = {k: [round(1e3 * float(v_), 4) for v_ in np.percentile(v, [25, 75])] for k, v in t.items()}
            print(json.dumps(dict(K=K, bodies_per_world=nb, feelers_per_world=per, ticks=a.ticks, reps=a.reps, gpu=torch.cuda.get_device_name(0), commit=commit,
                                  median_ms=med, quartiles_ms=quart, query_launches=launches,
                                  feelers_that_hit=int(result["feelers"][0].sum().item()), casts_that_hit=int(result["assembled"][0].sum().item()),
                                  equal=equal, device_skipped=b.counter("device_skipped"))), flush=True)
            del b
    stream.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
