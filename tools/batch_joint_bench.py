"""Times the joint rig of a batch, by the method of tools/batch_spring_bench.py - K worlds of sphere_pile(8, 8, 8) after --ticks ticks,
64 joints a world as 16 chains of five consecutive bodies (every joint's two anchors at the midpoint of its two bodies as they lie
when the rig is set: no gap to begin with), beta = 0.2, iters = 4, the library's work on one stream, the paths rotating their order
round by round, warm-up excluded, the median and the quartiles of --reps:
  (a) one solve_joints_dev(dt, 4): one launch;
  (b) beside it, one apply_springs_dev of a spring rig of the same ends (rest length 0, weak gains), on a batch of its own: two launches;
  (c) one step(1) of that batch: the tick the joints ride ahead of;
  (d) rollout_dev of T = 32 ticks that traces x of 16 bodies a world, on the batch with the joint rig;
  (e) the same rollout on a batch without it.
Before the timed rounds, once and unclocked: the impulses of (a) against the numpy restatement of the header's definition
(tests/batch_joint_cases.py) for the first 4 worlds, equal bytes; and the largest anchor gap |C| over the rig after 32 ticks of (d)
and of (e), from state().  Run by hand; prints one JSON line per K."""
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
from tests import batch_joint_cases as JC  # noqa: E402

f32 = np.float32
T = 32


def inverse_rotate(q, r):
    """r in the frame of q = (s, x, y, z), float64"""
    s, v = q[:, 0:1], -q[:, 1:4]
    return np.cross(v, np.cross(v, r) + r * s) * 2.0 + r


def full_state(b, worlds=None):
    """what the restatement reads: state() and get()'s inverse mass and inertia, every body (or the first `worlds` worlds')"""
    n = len(b) if worlds is None else sum(b.world_len(k) for k in range(worlds))
    lens = [b.world_len(k) for k in range(b.n_worlds)]
    w = np.concatenate([np.full(m, k, np.int32) for k, m in enumerate(lens)])[:n]
    bd = np.concatenate([np.arange(m, dtype=np.int32) for m in lens])[:n]
    st = {k: v[:n] for k, v in b.state().items()}
    got = b.get(w, bd)
    st["inv_mass"], st["inv_moment"] = got["inv_mass"], got["inv_moment"]
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[256])
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--iters", type=int, default=4)
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
            bj, bs, b0 = (mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K) for _ in range(3))
            for b in (bj, bs, b0):
                b.step(dt, iters, a.ticks)
            rig = JC.chains_rig(K, nb)
            per = len(rig) // K
            st = bj.state()
            x = (st["x"] + st["delta"]).astype(np.float64)
            ga, gb = rig["world"] * nb + rig["body"], rig["world"] * nb + rig["other"]
            mid = (x[ga] + x[gb]) / 2
            rig["pa"] = inverse_rotate(st["q"][ga].astype(np.float64), mid - x[ga])
            rig["pb"] = inverse_rotate(st["q"][gb].astype(np.float64), mid - x[gb])
            bj.set_joints(rig)
            bs.set_springs(rig["world"], rig["body"], other=rig["other"], pa=rig["pa"], pb=rig["pb"], rest=0.0, k=1e-3, c=1e-4)
            lens = [nb] * K
            body = torch.from_numpy(np.concatenate([k * nb + np.arange(16) * 5 for k in range(K)]).astype(np.int32)).cuda()
            xs = torch.empty((T, len(body), 3), dtype=torch.float32, device="cuda")
            imp = torch.empty((len(rig), 3), dtype=torch.float32, device="cuda")

            def sync():
                stream.synchronize()

            def solve_joints():
                bj.solve_joints_dev(dt, a.iters)

            def apply_springs():
                bs.apply_springs_dev(dt)

            def step_1():
                bs.step(dt, iters, 1)

            def rollout_joints():
                bj.rollout_dev(T, dt, iters, body=body, x=xs)

            def rollout_plain():
                b0.rollout_dev(T, dt, iters, body=body, x=xs)

            sync()
            # once, unclocked: (a)'s impulses against the definition restated on the host, the first 4 worlds
            head = 4 * per
            st4 = full_state(bj, 4)
            imp.fill_(float("nan"))
            bj.solve_joints_dev(dt, a.iters, impulses_dev=imp)
            sync()
            want = JC.solve(rig[:head], dt, a.iters, st4, lens[:4])
            after = full_state(bj, 4)
            equal = dict(impulses=imp.cpu().numpy()[:head].tobytes() == want[2].tobytes(), v=after["v"].tobytes() == want[0].tobytes(),
                         omega=after["omega"].tobytes() == want[1].tobytes())
            gap0 = float(JC.gaps(rig[:head], st4, lens[:4]).max())
            # ... and the gaps behind 32 ticks with and without the joints (every world of the batch; b0 carries no rig: the gaps its bodies would have)
            rollout_joints()
            rollout_plain()
            sync()
            launches_roll = bj.counter("rollout_launches")

            def all_gaps(b):
                s = b.state()
                xx = (s["x"] + s["delta"]).astype(np.float64)
                q = s["q"].astype(np.float64)

                def rot(qq, r):
                    sc_, v = qq[:, 0:1], qq[:, 1:4]
                    return np.cross(v, np.cross(v, r) + r * sc_) * 2.0 + r
                return np.linalg.norm((xx[gb] + rot(q[gb], rig["pb"].astype(np.float64))) - (xx[ga] + rot(q[ga], rig["pa"].astype(np.float64))), axis=1)
            gap_with, gap_without = all_gaps(bj), all_gaps(b0)
            fns = (solve_joints, apply_springs, step_1, rollout_joints, rollout_plain)
            t = {fn.__name__: [] for fn in fns}
            for rep in range(a.warmup + a.reps):
                for j in range(len(fns)):
                    fn = fns[(rep + j) % len(fns)]
                    sync()
                    t0 = time.perf_counter()
                    fn()
                    sync()
                    if rep >= a.warmup:
                        t[fn.__name__].append(time.perf_counter() - t0)
            launches = {}
            for fn, b in ((solve_joints, bj), (apply_springs, bs)):   # (unclocked)
                fn()
                launches[fn.__name__] = b.counter("drive_launches")
            sync()
            med = {key: round(1e3 * float(np.median(val)), 4) for key, val in t.items()}
            quart = {key: [round(1e3 * float(v_), 4) for v_ in np.percentile(val, [25, 75])] for key, val in t.items()}
            print(json.dumps(dict(K=K, bodies_per_world=nb, joints_per_world=per, iters=a.iters, T=T, ticks=a.ticks, reps=a.reps, gpu=torch.cuda.get_device_name(0),
                                  commit=commit, median_ms=med, quartiles_ms=quart, drive_launches=launches, rollout_launches_with_joints=launches_roll,
                                  equal=equal, gap_when_set=gap0, max_gap_after_T_with_joints=float(gap_with.max()), max_gap_after_T_without=float(gap_without.max()),
                                  joints_skipped=bj.counter("joints_skipped"), capacity_retries=[bj.counter("capacity_retries"), b0.counter("capacity_retries")])), flush=True)
            del bj, bs, b0
    stream.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
