"""Times the slider encoders of a batch, by the method and the rig of tools/batch_slider_bench.py - K worlds of sphere_pile(8, 8, 8) after
--ticks ticks, 64 sliders a world as 16 chains of five consecutive bodies, placed by slider_frames, every other slider limited to
[-0.3, 0.4], the others motorised without a cap with seeded targets, beta = 0.2, the library's work on one stream, the paths rotating
their order round by round, warm-up excluded, the median and the quartiles of --reps:
  (a) one read_sliders_dev: one launch;
  (b) beside it, one solve_sliders_dev(dt, 4, row 0) on a batch of its own: one launch;
  (c) what a caller needs for d today: gather_state of x and q of both ends of every slider and a torch expression that turns anchors
      and axis by q and takes dot(Pb - Pa, A);
  (d) rollout_dev of T = 64 ticks that traces x of 16 bodies a world with the readings table off;
  (e) the same rollout on a twin whose table has T rows of readings (32 bytes an entry);
  (f) the same on a twin whose table has T rows in the full format (64 bytes: the reading and the impulses of the tick's solve).
Before the timed rounds, once and unclocked: the readings of (a) against the numpy restatement of the header's definition
(tests/batch_slider_read_cases.py) for the first 4 worlds, equal bytes; d of (c) against d of (a); and rows 0 and T - 1 of (e)'s table
against read_sliders_dev of a twin driven by the defining loop's calls.  The kernels' own times are not measured here.  Run by hand;
prints one JSON line per K."""
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
from tests import batch_slider_cases as LC  # noqa: E402
from tests import batch_slider_read_cases as SR  # noqa: E402

f32 = np.float32
T = 64


def rotate(q, p):
    """p turned by the unit quaternions q = (s, v), rows: p + 2 cross(v, cross(v, p) + s p)"""
    s, v = q[:, :1], q[:, 1:]
    return p + 2.0 * torch.linalg.cross(v, torch.linalg.cross(v, p) + s * p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[256])
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=21)
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
            br, bs, b_off, b_read, b_full, b_loop = (mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K) for _ in range(6))
            every = (br, bs, b_off, b_read, b_full, b_loop)
            for b in every:
                b.step(dt, iters, a.ticks)
            lens = [nb] * K
            rig = LC.place(LC.chains_rig(K, nb), br.state(), lens, seed=11)
            per = len(rig) // K
            n = len(rig)
            W = np.random.default_rng(12).uniform(-1.5, 1.5, (T, n)).astype(f32)
            for b in every:
                b.set_sliders(rig)
                b.set_slider_targets(W)
            b_read.set_slider_trace(T)
            b_full.set_slider_trace(T, full=True)
            body = torch.from_numpy(np.concatenate([k * nb + np.arange(16) * 5 for k in range(K)]).astype(np.int32)).cuda()
            xs = torch.empty((T, len(body), 3), dtype=torch.float32, device="cuda")
            out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
            assert np.all(rig["other"] >= 0)
            ends = torch.from_numpy(np.concatenate([rig["world"] * nb + rig["body"], rig["world"] * nb + rig["other"]]).astype(np.int32)).cuda()
            ex = torch.empty((2 * n, 3), dtype=torch.float32, device="cuda")
            eq = torch.empty((2 * n, 4), dtype=torch.float32, device="cuda")
            pa, pb, ax = (torch.from_numpy(np.ascontiguousarray(rig[k])).cuda() for k in ("pa", "pb", "ax"))
            d_host = torch.empty(n, dtype=torch.float32, device="cuda")

            def sync():
                stream.synchronize()

            def read_sliders():
                br.read_sliders_dev(out)

            def solve_sliders():
                bs.solve_sliders_dev(dt, a.iters, 0)

            def gather_and_torch():
                br.gather_state(ends, x=ex, q=eq)
                A = rotate(eq[:n], ax)
                C = (ex[n:] + rotate(eq[n:], pb)) - (ex[:n] + rotate(eq[:n], pa))
                torch.sum(C * A, dim=1, out=d_host)

            def rollout_off():
                b_off.rollout_dev(T, dt, iters, body=body, x=xs)

            def rollout_reading():
                b_read.rollout_dev(T, dt, iters, body=body, x=xs)

            def rollout_full():
                b_full.rollout_dev(T, dt, iters, body=body, x=xs)

            sync()
            # once, unclocked: (a)'s readings against the definition restated on the host, the first 4 worlds; (c)'s d beside (a)'s
            head = 4 * per
            first = sum(lens[:4])
            st4 = {k: v[:first] for k, v in br.state().items()}
            out.fill_(float("nan"))
            read_sliders()
            gather_and_torch()
            sync()
            want = SR.readings(rig[:head], st4, lens[:4])
            equal = dict(readings=out.cpu().numpy()[:head].tobytes() == want.tobytes())
            d_torch_off = float((d_host - out[:, 0]).abs().max().item())
            # ... and rows 0 and T - 1 of (e)'s table against the defining loop's calls on a twin
            rollout_reading()
            rows = {}
            for t in range(T):
                b_loop.solve_sliders_dev(dt, iters, t)
                b_loop.step(dt, iters, 1)
                if t in (0, T - 1):
                    rows[t] = torch.empty((n, 8), dtype=torch.float32, device="cuda")
                    b_loop.read_sliders_dev(rows[t])
            sync()
            table = b_read.slider_trace()
            equal["row_0"] = SR.words(table[0]).tobytes() == rows[0].cpu().numpy().tobytes()
            equal["row_last"] = SR.words(table[T - 1]).tobytes() == rows[T - 1].cpu().numpy().tobytes()
            launches_roll = dict(off=None, reading=b_read.counter("rollout_launches"))
            fns = (read_sliders, solve_sliders, gather_and_torch, rollout_off, rollout_reading, rollout_full)
            t_ = {fn.__name__: [] for fn in fns}
            for rep in range(a.warmup + a.reps):
                for j in range(len(fns)):
                    fn = fns[(rep + j) % len(fns)]
                    sync()
                    t0 = time.perf_counter()
                    fn()
                    sync()
                    if rep >= a.warmup:
                        t_[fn.__name__].append(time.perf_counter() - t0)
            launches = {}
            for fn, b in ((read_sliders, br), (solve_sliders, bs)):   # (unclocked)
                fn()
                launches[fn.__name__] = b.counter("drive_launches")
            sync()
            launches_roll["off"], launches_roll["full"] = b_off.counter("rollout_launches"), b_full.counter("rollout_launches")
            med = {key: round(1e3 * float(np.median(val)), 4) for key, val in t_.items()}
            quart = {key: [round(1e3 * float(v_), 4) for v_ in np.percentile(val, [25, 75])] for key, val in t_.items()}
            print(json.dumps(dict(K=K, bodies_per_world=nb, sliders_per_world=per, iters=a.iters, T=T, ticks=a.ticks, reps=a.reps, gpu=torch.cuda.get_device_name(0),
                                  commit=commit, median_ms=med, quartiles_ms=quart, drive_launches=launches, rollout_launches=launches_roll, equal=equal,
                                  largest_d_torch_minus_d_read=d_torch_off, d_range_over_T=[float(table["d"].min()), float(table["d"].max())],
                                  largest_abs_rate=float(np.abs(table["rate"]).max()), largest_off_axis_gap=float(np.abs(table["off"]).max()),
                                  largest_frame_error=float(np.abs(table["e"]).max()),
                                  capacity_retries=[b.counter("capacity_retries") for b in (b_off, b_read, b_full)])), flush=True)
            del br, bs, b_off, b_read, b_full, b_loop, every
    stream.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
