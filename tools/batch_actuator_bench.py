"""Times one iteration of an actuator loop on a batch whose controls live on the device, in the setting of
tools/batch_feeler_bench.py - K worlds of sphere_pile(8, 8, 8) after --ticks ticks, 64 actuators a world (16 bodies with four thrusters
each: arms on the body's surface, directions in the body's frame, a clamp of [-1, 1]), impulse mode, the library's work and torch's
on one stream, the paths rotating their order round by round, warm-up excluded, the median and the quartiles of --reps - two ways:
  (a) actuate_dev of a rig set once: one launch;
  (b) the assembly a caller needs without the rig: gather_state of the actuator bodies (q), a torch expression that clamps u, turns d
      and p by q and takes the cross product, index_add_ of the wrenches per body, apply_impulses_dev of the sums.  ((b)'s rotate is
      torch's arithmetic and index_add_ decides the order of a body's sum: its velocities are close to (a)'s, not defined to the bit.)
Before the timed rounds the wrenches of (a) are compared with the numpy restatement of the header's definition from state(): equal
bytes.  The controls are small, so that the velocities stay where they were over the rounds.  Run by hand; prints one JSON line per K."""
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


def np_cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def np_rotate(q, r):
    """Rotation::rotate_vector in f32, operation by operation"""
    s, v = q[:, 0:1], q[:, 1:4]
    return np_cross(v, np_cross(v, r) + r * s) * np.float32(2.0) + r


def torch_rotate(q, r):
    s, v = q[:, 0:1], q[:, 1:4]
    return torch.linalg.cross(v, torch.linalg.cross(v, r) + r * s) * 2.0 + r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[256])
    ap.add_argument("--bodies", type=int, default=16, help="actuated bodies a world")
    ap.add_argument("--each", type=int, default=4, help="actuators a body")
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
            per, n = a.bodies * a.each, K * a.bodies * a.each
            rng = np.random.default_rng(2)
            local = np.tile(np.repeat(rng.choice(nb, a.bodies, replace=False), a.each), K).astype(np.int32)
            world_np = np.repeat(np.arange(K, dtype=np.int32), per)
            body_np = (world_np * nb + local).astype(np.int32)
            d_np = rng.normal(0, 1, (n, 3))
            d_np = (d_np / np.linalg.norm(d_np, axis=1, keepdims=True)).astype(np.float32)
            p_np = rng.normal(0, 1, (n, 3))
            p_np = (0.5 * p_np / np.linalg.norm(p_np, axis=1, keepdims=True)).astype(np.float32)
            gain_np = rng.uniform(0.5, 1.5, n).astype(np.float32)
            u_np = rng.uniform(-2e-3, 2e-3, n).astype(np.float32)
            lo, hi = np.float32(-1e-3), np.float32(1e-3)
            uniq_np, slot_np = np.unique(body_np, return_inverse=True)
            m = len(uniq_np)
            d_body, d_uniq = torch.from_numpy(body_np).cuda(), torch.from_numpy(uniq_np.astype(np.int32)).cuda()
            d_slot = torch.from_numpy(slot_np.astype(np.int64)).cuda()
            d_p, d_d = torch.from_numpy(p_np).cuda(), torch.from_numpy(d_np).cuda()
            d_gain, d_u = torch.from_numpy(gain_np).cuda(), torch.from_numpy(u_np).cuda()
            q = torch.empty((n, 4), dtype=torch.float32, device="cuda")
            wrench = torch.empty((n, 6), dtype=torch.float32, device="cuda")
            b.set_actuators(world_np, local, p=p_np, d=d_np, gain=gain_np, lo=lo, hi=hi)

            def sync():
                stream.synchronize()

            def rig():
                b.actuate_dev(d_u, mgf_amd.ACTUATE_IMPULSE)

            def assembled():
                b.gather_state(d_body, q=q)
                s = (d_gain * torch.clamp(d_u, float(lo), float(hi))).unsqueeze(1)
                L = torch_rotate(q, d_d) * s
                A = torch.linalg.cross(torch_rotate(q, d_p), L)
                Ls = torch.zeros((m, 3), dtype=torch.float32, device="cuda").index_add_(0, d_slot, L)
                As = torch.zeros((m, 3), dtype=torch.float32, device="cuda").index_add_(0, d_slot, A)
                b.apply_impulses_dev(d_uniq, Ls, As)

            sync()
            # once, unclocked: (a)'s wrenches against the header's definition restated on the host from state()
            wrench.fill_(float("nan"))
            b.actuate_dev(d_u, mgf_amd.ACTUATE_IMPULSE, wrenches_out=wrench)
            sync()
            qs = b.state()["q"][body_np]
            s_np = gain_np * np.clip(u_np, lo, hi)
            L_np = np_rotate(qs, d_np) * s_np[:, None]
            want = np.concatenate([L_np, np_cross(np_rotate(qs, p_np), L_np)], axis=1).astype(np.float32)
            equal = dict(restatement_from_state=wrench.cpu().numpy().tobytes() == want.tobytes())
            fns = (rig, assembled)
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
                launches[fn.__name__] = b.counter("drive_launches")
            sync()
            med = {k: round(1e3 * float(np.median(v)), 4) for k, v in t.items()}
            quart = {k: [round(1e3 * float(v_), 4) for v_ in np.percentile(v, [25, 75])] for k, v in t.items()}
            print(json.dumps(dict(K=K, bodies_per_world=nb, actuators_per_world=per, actuated_bodies=m, ticks=a.ticks, reps=a.reps, gpu=torch.cuda.get_device_name(0),
                                  commit=commit, median_ms=med, quartiles_ms=quart, drive_launches=launches, equal=equal,
                                  actuators_skipped=b.counter("actuators_skipped"), device_skipped=b.counter("device_skipped"))), flush=True)
            del b
    stream.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
