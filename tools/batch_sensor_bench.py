"""Times one iteration of a sensor loop on a batch whose hits are consumed on the device, in the setting of
tools/batch_device_query_bench.py - K worlds of sphere_pile(8, 8, 8) after --ticks ticks, 64 rays a world, the library's work and
torch's on one stream, the paths rotating their order round by round, warm-up excluded, the median and the quartiles of --reps - two ways:
  (a) cast_sensors_dev of a rig set once - the same bodies, a ray from 20 above each in its own frame - and the torch reduction of the
      hits (hits per world, the nearest t per world);
  (b) that tool's path (b) as it stands: gather_state of the sensor bodies, a torch expression that turns it into the particles,
      raycast_dev with the fixed layout, the same reduction.  ((b) does not turn its rays by q: it is the cheaper assembly.)
Before the timed rounds the hits of (a) are compared with cast_sensors and with raycast of particles made on the host from state():
equal bytes.  Run by hand; prints one JSON line per K."""
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


def host_particles(st, g, p, d):
    """P = x + rotate(q, p), D = rotate(q, d) in f32, operation by operation (Rotation::rotate_vector)"""
    def cross(a, b):
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)

    def rotate(q, r):
        s, v = q[:, 0:1], q[:, 1:4]
        return cross(v, cross(v, r) + r * s) * np.float32(2.0) + r
    x, q = st["x"][g], st["q"][g]
    return x + rotate(q, p), rotate(q, d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[256])
    ap.add_argument("--rays", type=int, default=64, help="rays a world")
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
            per, n = a.rays, K * a.rays
            rng = np.random.default_rng(2)
            # the sensors: `per` bodies of every world, a ray from 20 above each, down and a little to the side
            local = np.tile(rng.choice(nb, per, replace=False), K).astype(np.int32)
            world_np = np.repeat(np.arange(K, dtype=np.int32), per)
            body_np = (world_np * nb + local).astype(np.int32)
            dir_np = np.concatenate([rng.normal(0, 0.05, (n, 1)), np.full((n, 1), -1.0), rng.normal(0, 0.05, (n, 1))], axis=1).astype(np.float32)
            up_np = np.tile(np.float32([0.0, 20.0, 0.0]), (n, 1))
            d_body = torch.from_numpy(body_np).cuda()
            d_dir = torch.from_numpy(dir_np).cuda()
            up = torch.tensor([0.0, 20.0, 0.0], dtype=torch.float32, device="cuda")
            inf = torch.full((n, 1), float("inf"), dtype=torch.float32, device="cuda")
            x = torch.empty((n, 3), dtype=torch.float32, device="cuda")
            out_a = torch.empty((n, 7), dtype=torch.int32, device="cuda")
            out_b = torch.empty((n, 7), dtype=torch.int32, device="cuda")
            b.set_sensors(world_np, local, up_np, dir_np, float("inf"), False)     # (as (b): nothing ignored)
            result = {}

            def sync():
                stream.synchronize()

            def reduce(hits, key):
                h = hits.view(K, per, 7)
                t = torch.where(h[..., 0] >= 0, h[..., 6].view(torch.float32), torch.full((), float("inf"), device="cuda"))
                result[key] = ((h[..., 0] >= 0).sum(dim=1), t.min(dim=1).values)

            def sensors():
                b.cast_sensors_dev(out_a)
                reduce(out_a, "sensors")

            def assembled():
                b.gather_state(d_body, x=x)
                b.raycast_dev(None, torch.cat([x + up, d_dir, inf], dim=1), out_b)
                reduce(out_b, "assembled")

            sync()
            # once, unclocked: (a) against the host-memory form and against raycast of particles made on the host from state()
            out_a.fill_(0x5A5A5A5A)
            sensors()
            sync()
            got = out_a.cpu().numpy().tobytes()
            P, D = host_particles(b.state(), body_np, up_np, dir_np)
            equal = dict(cast_sensors=got == b.cast_sensors().tobytes(), raycast_from_state=got == b.raycast(world_np, P, D).tobytes())
            fns = (sensors, assembled)
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
            quart = {k: [round(1e3 * float(q), 4) for q in np.percentile(v, [25, 75])] for k, v in t.items()}
            print(json.dumps(dict(K=K, bodies_per_world=nb, rays_per_world=per, ticks=a.ticks, reps=a.reps, gpu=torch.cuda.get_device_name(0), commit=commit,
                                  median_ms=med, quartiles_ms=quart, query_launches=launches,
                                  sensors_that_hit=int(result["sensors"][0].sum().item()), rays_that_hit=int(result["assembled"][0].sum().item()),
                                  equal=equal, device_skipped=b.counter("device_skipped"))), flush=True)
            del b
    stream.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
