"""Times one application of a spring rig on a batch, in the setting of tools/batch_actuator_bench.py - K worlds of sphere_pile(8, 8, 8)
after --ticks ticks, 64 springs a world (32 bodies, every body an end of four springs: arms on the bodies' surfaces, a rest length near
the distance, weak gains so that the velocities stay where they were over the rounds), the library's work and torch's on one stream,
the paths alternating their order round by round, warm-up excluded, the median and the quartiles of --reps - two ways:
  (a) apply_springs_dev of a rig set once: two launches;
  (b) the assembly a caller needs without the rig: gather_state of both ends (x, q, v, omega), a torch expression that turns two arms
      by two quaternions, forms point velocities, a length, a unit vector, a clamp and two cross products, index_add_ of the impulses
      per body, apply_impulses_dev of the sums.  ((b)'s arithmetic is torch's and index_add_ decides the order of a body's sum: its
      velocities are close to (a)'s, not defined to the bit.)
Before the timed rounds the wrenches of (a) are compared with the numpy restatement of the header's definition from state(): equal
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

f32 = np.float32


def np_cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def np_dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def np_rotate(q, r):
    """Rotation::rotate_vector in f32, operation by operation"""
    s, v = q[:, 0:1], q[:, 1:4]
    return np_cross(v, np_cross(v, r) + r * s) * f32(2.0) + r


def np_wrenches(st, ga, gb, pa, pb, rest, k, c, lo, hi, h):
    """the header's definition for springs between two bodies, in f32 (no skips expected here)"""
    x = (st["x"] + st["delta"]).astype(f32)
    ra, rb = np_rotate(st["q"][ga], pa), np_rotate(st["q"][gb], pb)
    Pa, Pb = x[ga] + ra, x[gb] + rb
    Va, Vb = st["v"][ga] + np_cross(st["omega"][ga], ra), st["v"][gb] + np_cross(st["omega"][gb], rb)
    d = Pb - Pa
    ln = np.sqrt(np_dot(d, d))
    n = d / ln[:, None]
    f = k * (ln - rest) + c * np_dot(Vb - Va, n)
    f = np.where(f < lo, lo, f)
    f = np.where(f > hi, hi, f)
    L = n * (f * f32(h))[:, None]
    Lb = -L
    return np.concatenate([L, np_cross(ra, L), Lb, np_cross(rb, Lb)], axis=1).astype(f32)


def torch_rotate(q, r):
    s, v = q[:, 0:1], q[:, 1:4]
    return torch.linalg.cross(v, torch.linalg.cross(v, r) + r * s) * 2.0 + r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[256])
    ap.add_argument("--springs", type=int, default=64, help="springs a world")
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
            per, n = a.springs, K * a.springs
            rng = np.random.default_rng(2)
            bodies = rng.choice(nb, per // 2, replace=False)
            # a ring with two strands: body j is tied to j + 1 and j + 3 - every body an end of four springs
            la = np.concatenate([bodies, bodies]).astype(np.int32)
            lb = np.concatenate([np.roll(bodies, -1), np.roll(bodies, -3)]).astype(np.int32)
            world_np = np.repeat(np.arange(K, dtype=np.int32), per)
            la, lb = np.tile(la, K), np.tile(lb, K)
            ga, gb = (world_np * nb + la).astype(np.int32), (world_np * nb + lb).astype(np.int32)
            pa = rng.normal(0, 1, (n, 3))
            pa = (0.5 * pa / np.linalg.norm(pa, axis=1, keepdims=True)).astype(f32)
            pb = rng.normal(0, 1, (n, 3))
            pb = (0.5 * pb / np.linalg.norm(pb, axis=1, keepdims=True)).astype(f32)
            st = b.state()
            dist = np.linalg.norm((st["x"] + st["delta"])[gb] - (st["x"] + st["delta"])[ga], axis=1)
            rest = (dist * rng.uniform(0.9, 1.1, n)).astype(f32)
            k_np, c_np = rng.uniform(1e-3, 2e-3, n).astype(f32), rng.uniform(1e-4, 2e-4, n).astype(f32)
            lo, hi = f32(-1e-2), f32(1e-2)
            both = np.concatenate([ga, gb])
            uniq_np, slot_np = np.unique(both, return_inverse=True)
            m = len(uniq_np)
            d_both, d_uniq = torch.from_numpy(both.astype(np.int32)).cuda(), torch.from_numpy(uniq_np.astype(np.int32)).cuda()
            d_slot = torch.from_numpy(slot_np.astype(np.int64)).cuda()
            d_pa, d_pb = torch.from_numpy(pa).cuda(), torch.from_numpy(pb).cuda()
            d_rest, d_k, d_c = torch.from_numpy(rest).cuda(), torch.from_numpy(k_np).cuda(), torch.from_numpy(c_np).cuda()
            x = torch.empty((2 * n, 3), dtype=torch.float32, device="cuda")
            q = torch.empty((2 * n, 4), dtype=torch.float32, device="cuda")
            v, om = torch.empty_like(x), torch.empty_like(x)
            wrench = torch.empty((n, 12), dtype=torch.float32, device="cuda")
            b.set_springs(world_np, la, other=lb, pa=pa, pb=pb, rest=rest, k=k_np, c=c_np, lo=lo, hi=hi)

            def sync():
                stream.synchronize()

            def rig():
                b.apply_springs_dev(dt)

            def assembled():
                b.gather_state(d_both, x=x, q=q, v=v, omega=om)
                ra, rb = torch_rotate(q[:n], d_pa), torch_rotate(q[n:], d_pb)
                d = (x[n:] + rb) - (x[:n] + ra)
                ln = torch.linalg.vector_norm(d, dim=1)
                nn = d / ln.unsqueeze(1)
                rel = (v[n:] + torch.linalg.cross(om[n:], rb)) - (v[:n] + torch.linalg.cross(om[:n], ra))
                f = torch.clamp(d_k * (ln - d_rest) + d_c * (rel * nn).sum(dim=1), float(lo), float(hi))
                L = nn * (f * dt).unsqueeze(1)
                lin = torch.cat([L, -L])
                ang = torch.cat([torch.linalg.cross(ra, L), torch.linalg.cross(rb, -L)])
                Ls = torch.zeros((m, 3), dtype=torch.float32, device="cuda").index_add_(0, d_slot, lin)
                As = torch.zeros((m, 3), dtype=torch.float32, device="cuda").index_add_(0, d_slot, ang)
                b.apply_impulses_dev(d_uniq, Ls, As)

            sync()
            # once, unclocked: (a)'s wrenches against the header's definition restated on the host from state()
            wrench.fill_(float("nan"))
            st = b.state()
            b.apply_springs_dev(dt, wrenches_out=wrench)
            sync()
            want = np_wrenches(st, ga, gb, pa, pb, rest, k_np, c_np, lo, hi, dt)
            got = wrench.cpu().numpy()
            equal = dict(restatement_from_state=got.tobytes() == want.tobytes())
            clamped = float(np.mean(np.abs(np.linalg.norm(got[:, 0:3], axis=1) - hi * f32(dt)) < 1e-9))
            fns = (rig, assembled)
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
                launches[fn.__name__] = b.counter("drive_launches")
            sync()
            med = {key: round(1e3 * float(np.median(val)), 4) for key, val in t.items()}
            quart = {key: [round(1e3 * float(v_), 4) for v_ in np.percentile(val, [25, 75])] for key, val in t.items()}
            print(json.dumps(dict(K=K, bodies_per_world=nb, springs_per_world=per, bodies_with_an_end=m, ticks=a.ticks, reps=a.reps, gpu=torch.cuda.get_device_name(0),
                                  commit=commit, median_ms=med, quartiles_ms=quart, drive_launches=launches, equal=equal, clamped_fraction=round(clamped, 3),
                                  springs_skipped=b.counter("springs_skipped"), device_skipped=b.counter("device_skipped"))), flush=True)
            del b
    stream.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
