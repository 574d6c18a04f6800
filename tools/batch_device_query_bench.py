"""Times one iteration of a sensor loop on a batch whose rays are computed on the device and whose hits are consumed there:
gather_state of the sensor bodies into a CUDA tensor, a torch expression that turns it into --rays particles a world, the ray cast, a
torch reduction of the hits (hits per world, the nearest t per world) - three ways:
  (a) raycast_dev with a world tensor (the plan is built on the device);
  (b) raycast_dev with the fixed layout (world=None: no plan);
  (c) the host-memory raycast with what a caller needs around it today: .cpu() of the particles, the call, torch.from_numpy(...).cuda()
      of the hits.  (c) is the yardstick.
K worlds of sphere_pile(8, 8, 8) (512 spheres) after --ticks ticks, 64 rays a world: the README's case of tools/batch_query_bench.py.
The library's work and torch's share one stream (mgf_ctx_set_stream), so (a) and (b) need no wait inside the iteration.  Wall clock from
the first call to a completed synchronize of that stream, every interval with a clock of its own, the three paths rotating their order
round by round, warm-up excluded, the median and the quartiles of --reps.  Before the timed rounds (a) and (b) are compared with (c):
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
            body_np = (np.repeat(np.arange(K), per) * nb + np.tile(rng.choice(nb, per, replace=False), K)).astype(np.int32)
            world_np = np.repeat(np.arange(K, dtype=np.int32), per)
            d_body, d_world = torch.from_numpy(body_np).cuda(), torch.from_numpy(world_np).cuda()
            d_dir = torch.from_numpy(np.concatenate([rng.normal(0, 0.05, (n, 1)), np.full((n, 1), -1.0), rng.normal(0, 0.05, (n, 1))], axis=1).astype(np.float32)).cuda()
            up = torch.tensor([0.0, 20.0, 0.0], dtype=torch.float32, device="cuda")
            inf = torch.full((n, 1), float("inf"), dtype=torch.float32, device="cuda")
            x = torch.empty((n, 3), dtype=torch.float32, device="cuda")
            out = torch.empty((n, 7), dtype=torch.int32, device="cuda")
            result = {}

            def sync():
                stream.synchronize()

            def particles():
                b.gather_state(d_body, x=x)
                return torch.cat([x + up, d_dir, inf], dim=1)

            def reduce(hits, key):
                h = hits.view(K, per, 7)
                t = torch.where(h[..., 0] >= 0, h[..., 6].view(torch.float32), torch.full((), float("inf"), device="cuda"))
                result[key] = ((h[..., 0] >= 0).sum(dim=1), t.min(dim=1).values)

            def dev_world():
                b.raycast_dev(d_world, particles(), out)
                reduce(out, "dev_world")

            def dev_fixed():
                b.raycast_dev(None, particles(), out)
                reduce(out, "dev_fixed")

            def host():
                parts = particles().cpu().numpy()
                got = b.raycast(world_np, parts[:, 0:3], parts[:, 3:6], parts[:, 6])
                reduce(torch.from_numpy(got.view(np.int32).reshape(n, 7)).cuda(), "host")

            sync()
            # once, unclocked: the three give the same hits
            host()
            sync()
            want = b.raycast(world_np, *(lambda p: (p[:, 0:3], p[:, 3:6], p[:, 6]))(particles().cpu().numpy()))
            equal = {}
            for fn in (dev_world, dev_fixed):
                out.fill_(0x5A5A5A5A)
                fn()
                sync()
                equal[fn.__name__] = out.cpu().numpy().tobytes() == want.tobytes() and all(torch.equal(u, v) for u, v in zip(result[fn.__name__], result["host"]))
            fns = (dev_world, dev_fixed, host)
            t = {fn.__name__: [] for fn in fns}
            for rep in range(a.warmup + a.reps):
                for k in range(3):
                    fn = fns[(rep + k) % 3]
                    sync()
                    t0 = time.perf_counter()
                    fn()
                    sync()
                    if rep >= a.warmup:
                        t[fn.__name__].append(time.perf_counter() - t0)
            launches = {}
            for fn in (dev_world, dev_fixed):   # (unclocked)
                fn()
                launches[fn.__name__] = b.counter("query_launches")
            sync()
            hits = int(result["host"][0].sum().item())
            med = {k: round(1e3 * float(np.median(v)), 4) for k, v in t.items()}
            quart = {k: [round(1e3 * float(q), 4) for q in np.percentile(v, [25, 75])] for k, v in t.items()}
            print(json.dumps(dict(K=K, bodies_per_world=nb, rays_per_world=per, ticks=a.ticks, reps=a.reps, gpu=torch.cuda.get_device_name(0), commit=commit,
                                  median_ms=med, quartiles_ms=quart, query_launches=launches, rays_that_hit=hits, equal_to_host=equal,
                                  device_skipped=b.counter("device_skipped"))), flush=True)
            del b
    stream.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
