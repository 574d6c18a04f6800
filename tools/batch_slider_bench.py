"""Times the slider rig of a batch, by the method of tools/batch_hinge_bench.py - K worlds of sphere_pile(8, 8, 8) after --ticks ticks,
64 sliders a world as 16 chains of five consecutive bodies, placed by slider_frames at the midpoint of each pair as the bodies lie when the
rig is set (no gap, aligned frames, d = 0), every other slider limited to [-0.3, 0.4], the others motorised without a cap with seeded
targets, beta = 0.2, iters = 4, the library's work on one stream, the paths rotating their order round by round, warm-up excluded, the
median and the quartiles of --reps:
  (a) one solve_sliders_dev(dt, 4, row 0): one launch;
  (b) beside it, one solve_hinges_dev(dt, 4, row 0) of a hinge rig on the same ends, anchors and axes, on a batch of its own: one launch;
  (c) one step(1) of that batch: the tick the sliders ride ahead of;
  (d) rollout_dev of T = 32 ticks that traces x of 16 bodies a world, on the batch with the slider rig and a table of T rows;
  (e) the same rollout on a batch without a rig.
Before the timed rounds, once and unclocked: the impulses, v and omega of (a) against the numpy restatement of the header's definition
(tests/batch_slider_cases.py) for the first 4 worlds, equal bytes; and the largest off-axis gap and frame error |e| over the rig after
32 ticks of (d) and of (e), from state().  Run by hand; prints one JSON line per K."""
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
from tests import batch_hinge_cases as HC  # noqa: E402
from tests import batch_slider_cases as LC  # noqa: E402

f32 = np.float32
T = 32


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
            bs, bh, b0 = (mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K) for _ in range(3))
            for b in (bs, bh, b0):
                b.step(dt, iters, a.ticks)
            lens = [nb] * K
            rig = LC.place(LC.chains_rig(K, nb), bs.state(), lens, seed=11)
            per = len(rig) // K
            W = np.random.default_rng(12).uniform(-1.5, 1.5, (T, len(rig))).astype(f32)
            bs.set_sliders(rig)
            bs.set_slider_targets(W)
            hinges = HC.chains_rig(K, nb)
            for k in ("pa", "pb", "ax", "ua", "bx", "ub"):
                hinges[k] = rig[k]
            bh.set_hinges(hinges)
            bh.set_hinge_targets(W)
            body = torch.from_numpy(np.concatenate([k * nb + np.arange(16) * 5 for k in range(K)]).astype(np.int32)).cuda()
            xs = torch.empty((T, len(body), 3), dtype=torch.float32, device="cuda")
            imp = torch.empty((len(rig), 8), dtype=torch.float32, device="cuda")

            def sync():
                stream.synchronize()

            def solve_sliders():
                bs.solve_sliders_dev(dt, a.iters, 0)

            def solve_hinges():
                bh.solve_hinges_dev(dt, a.iters, 0)

            def step_1():
                bh.step(dt, iters, 1)

            def rollout_sliders():
                bs.rollout_dev(T, dt, iters, body=body, x=xs)

            def rollout_plain():
                b0.rollout_dev(T, dt, iters, body=body, x=xs)

            sync()
            # once, unclocked: (a)'s impulses and velocities against the definition restated on the host, the first 4 worlds
            head = 4 * per
            st4 = full_state(bs, 4)
            imp.fill_(float("nan"))
            bs.solve_sliders_dev(dt, a.iters, 0, impulses_dev=imp)
            sync()
            want = LC.solve(rig[:head], dt, a.iters, W[0, :head], st4, lens[:4])
            after = full_state(bs, 4)
            equal = dict(impulses=imp.cpu().numpy()[:head].tobytes() == want[2].tobytes(), v=after["v"].tobytes() == want[0].tobytes(),
                         omega=after["omega"].tobytes() == want[1].tobytes())
            d0, off0, e0 = (float(np.abs(x).max()) for x in LC.travel(rig[:head], st4, lens[:4]))
            # ... and the gaps and frame errors behind 32 ticks with and without the sliders (b0 carries no rig: what its bodies would show)
            rollout_sliders()
            rollout_plain()
            sync()
            launches_roll = bs.counter("rollout_launches")
            d_with, off_with, e_with = LC.travel(rig, bs.state(), lens)
            d_without, off_without, e_without = LC.travel(rig, b0.state(), lens)
            limited = d_with[(rig["flags"] & LC.LIMIT) != 0]
            fns = (solve_sliders, solve_hinges, step_1, rollout_sliders, rollout_plain)
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
            for fn, b in ((solve_sliders, bs), (solve_hinges, bh)):   # (unclocked)
                fn()
                launches[fn.__name__] = b.counter("drive_launches")
            sync()
            med = {key: round(1e3 * float(np.median(val)), 4) for key, val in t.items()}
            quart = {key: [round(1e3 * float(v_), 4) for v_ in np.percentile(val, [25, 75])] for key, val in t.items()}
            print(json.dumps(dict(K=K, bodies_per_world=nb, sliders_per_world=per, iters=a.iters, T=T, ticks=a.ticks, reps=a.reps, gpu=torch.cuda.get_device_name(0),
                                  commit=commit, median_ms=med, quartiles_ms=quart, drive_launches=launches, rollout_launches_with_sliders=launches_roll,
                                  equal=equal, travel_when_set=d0, off_axis_gap_when_set=off0, frame_error_when_set=e0,
                                  max_off_axis_gap_after_T_with_sliders=float(off_with.max()), max_off_axis_gap_after_T_without=float(off_without.max()),
                                  max_frame_error_after_T_with_sliders=float(e_with.max()), max_frame_error_after_T_without=float(e_without.max()),
                                  limited_travel_after_T=[float(limited.min()), float(limited.max())],
                                  sliders_skipped=bs.counter("sliders_skipped"), capacity_retries=[bs.counter("capacity_retries"), b0.counter("capacity_retries")])), flush=True)
            del bs, bh, b0
    stream.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
