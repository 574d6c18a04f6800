"""Times a horizon of T ticks under T control vectors with a state trace AND the contact sensors' reports of every tick, in the setting
of tools/batch_rollout_bench.py - K worlds of sphere_pile(8, 8, 8) after --ticks ticks, 64 actuators a world (16 bodies with four
thrusters each, a clamp of [-1, 1] mN s), 64 contact sensors a world (16 bodies with four filters each: every record, the ground, any
body in the body's frame, one named neighbour), 16 traced bodies a world, impulse mode, one stream, wall clock from a synchronized stream
to a completed synchronize, the paths rotating their order round by round, warm-up excluded, the median and the quartiles of --reps:
  (a) one rollout_touches_dev, full reports (64 bytes) and short ones (16 bytes);
  (b) the loop that defines it: apply_springs_dev(dt) (the spring rig is empty: nothing is enqueued), actuate_dev(u[t]), step(dt, iters, 1),
      gather_state(row t), read_touches_dev(row t), T times;
  (c) rollout_dev alone: what the trace costs is (a) - (c).
Every timed call starts from the same state: the batch is copied back from a snapshot batch (copy_worlds, unclocked) before it.
Before the timed rounds (a)'s touch rows, traces and stats are compared with (b)'s from that state: equal bytes; the short rows are the
four words of the full ones.  Run by hand; prints one JSON line per K."""
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

TRACES = (("x", 3), ("q", 4), ("v", 3), ("omega", 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[256])
    ap.add_argument("--bodies", type=int, default=16, help="actuated bodies a world, and bodies with sensors")
    ap.add_argument("--each", type=int, default=4, help="actuators a body")
    ap.add_argument("--traced", type=int, default=16, help="traced bodies a world")
    ap.add_argument("--horizon", type=int, default=32, help="T")
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=31)
    a = ap.parse_args()
    ctx = mgf_amd.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    sc = scenes.sphere_pile(8, 8, 8)
    dt, iters, nb, T = float(sc["dt"]), sc["iters"], len(sc["comps"]), a.horizon
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
    except OSError:
        commit = ""
    with torch.cuda.stream(stream):
        for K in a.ks:
            snap = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
            snap.step(dt, iters, a.ticks)
            b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
            b.step(dt, iters, a.ticks)
            every = np.arange(K, dtype=np.int32)
            per, n = a.bodies * a.each, K * a.bodies * a.each
            rng = np.random.default_rng(2)
            local = np.tile(np.repeat(rng.choice(nb, a.bodies, replace=False), a.each), K).astype(np.int32)
            world_np = np.repeat(every, per)
            d_np = rng.normal(0, 1, (n, 3))
            d_np = (d_np / np.linalg.norm(d_np, axis=1, keepdims=True)).astype(np.float32)
            p_np = rng.normal(0, 1, (n, 3))
            p_np = (0.5 * p_np / np.linalg.norm(p_np, axis=1, keepdims=True)).astype(np.float32)
            gain_np = rng.uniform(0.5, 1.5, n).astype(np.float32)
            b.set_actuators(world_np, local, p=p_np, d=d_np, gain=gain_np, lo=np.float32(-1e-3), hi=np.float32(1e-3))
            # the sensors: four filters on each of a.bodies bodies of every world
            on = rng.choice(nb, a.bodies, replace=False).astype(np.int32)
            s_body = np.tile(np.repeat(on, 4), K)
            s_other = np.tile(np.stack([np.full(a.bodies, mgf_amd.TOUCH_ANY), np.full(a.bodies, mgf_amd.TOUCH_STATIC), np.full(a.bodies, mgf_amd.TOUCH_ANY_BODY),
                                        (on + 1) % nb], axis=1).reshape(-1), K).astype(np.int32)
            s_frame = np.tile(np.tile([False, False, True, False], a.bodies), K)
            b.set_touches(np.repeat(every, 4 * a.bodies), s_body, other=s_other, body_frame=s_frame)
            ns = b.touch_count()
            traced_np = (np.repeat(every, a.traced) * nb + np.tile(rng.choice(nb, a.traced, replace=False), K)).astype(np.int32)
            m = len(traced_np)
            d_u = torch.from_numpy(rng.uniform(-2e-3, 2e-3, (T, n)).astype(np.float32)).cuda()
            d_body = torch.from_numpy(traced_np).cuda()
            paths = ("touches_full", "touches_short", "loop", "rollout")
            out = {p: {k: torch.empty((T, m, c), dtype=torch.float32, device="cuda") for k, c in TRACES} for p in paths}
            touch = {p: torch.empty((T, ns, 4 if p == "touches_short" else 16), dtype=torch.int32, device="cuda") for p in paths[:3]}
            stats, extra = {}, {}

            def sync():
                stream.synchronize()

            def reset():
                b.copy_worlds(every, snap, every)
                sync()

            def touches_full():
                stats["touches_full"] = bytes(b.rollout_touches_dev(d_u, dt, iters, mgf_amd.ACTUATE_IMPULSE, body=d_body, touches=touch["touches_full"], **out["touches_full"]))

            def touches_short():
                stats["touches_short"] = bytes(b.rollout_touches_dev(d_u, dt, iters, mgf_amd.ACTUATE_IMPULSE, body=d_body, touches=touch["touches_short"], short=True,
                                                                     **out["touches_short"]))

            def rollout():
                stats["rollout"] = bytes(b.rollout_dev(d_u, dt, iters, mgf_amd.ACTUATE_IMPULSE, body=d_body, **out["rollout"]))

            def loop():
                o, st = out["loop"], b""
                for t in range(T):
                    b.apply_springs_dev(dt)
                    b.actuate_dev(d_u[t], mgf_amd.ACTUATE_IMPULSE)
                    st += bytes(b.step(dt, iters, 1))
                    b.gather_state(d_body, x=o["x"][t], q=o["q"][t], v=o["v"][t], omega=o["omega"][t])
                    b.read_touches_dev(touch["loop"][t])
                stats["loop"] = st

            fns = (touches_full, touches_short, loop, rollout)
            # once, unclocked: every path from the same state - touch rows, traces, stats and the state the batch is left in
            end = {}
            for fn in fns:
                reset()
                for o in out[fn.__name__].values():
                    o.fill_(float("nan"))
                if fn.__name__ in touch:
                    touch[fn.__name__].fill_(0x5A5A5A5A)
                retries = b.counter("capacity_retries")
                fn()
                sync()
                extra[fn.__name__] = dict(rollout_launches=b.counter("rollout_launches"), passes=1 + b.counter("capacity_retries") - retries)
                end[fn.__name__] = b"".join(v.tobytes() for v in b.state().values())
            full, short, ref = (touch[p].cpu().numpy() for p in paths[:3])
            equal = dict(touches_full=full.tobytes() == ref.tobytes(), touches_short=short.tobytes() == np.ascontiguousarray(ref[:, :, [0, 1, 7, 11]]).tobytes(),
                         traces=all(out[p][k].cpu().numpy().tobytes() == out["loop"][k].cpu().numpy().tobytes() for p in paths for k, _ in TRACES),
                         stats=all(stats[p] == stats["loop"] for p in paths), state=all(end[p] == end["loop"] for p in paths))
            touched = int((ref[:, :, 0] > 0).sum())
            retries0 = b.counter("capacity_retries")
            t = {fn.__name__: [] for fn in fns}
            for rep in range(a.warmup + a.reps):
                for k in range(len(fns)):
                    fn = fns[(rep + k) % len(fns)]
                    reset()
                    t0 = time.perf_counter()
                    fn()
                    sync()
                    if rep >= a.warmup:
                        t[fn.__name__].append(time.perf_counter() - t0)
            tick = b.counter("launches_per_tick")
            launches = {p: T * tick + extra[p]["rollout_launches"] for p in ("touches_full", "touches_short", "rollout")}
            launches["loop"] = T * (tick + mgf_amd.BATCH_ACTUATOR_LAUNCHES + 1 + mgf_amd.BATCH_TOUCH_LAUNCHES)
            # one host wait per pass: the passes of the untimed call (1 + the capacity re-runs it made)
            host_waits = {p: extra[p]["passes"] for p in ("touches_full", "touches_short", "rollout")}
            host_waits["loop"] = T
            med = {k: round(1e3 * float(np.median(v)), 4) for k, v in t.items()}
            quart = {k: [round(1e3 * float(v_), 4) for v_ in np.percentile(v, [25, 75])] for k, v in t.items()}
            print(json.dumps(dict(K=K, bodies_per_world=nb, actuators_per_world=per, sensors_per_world=ns // K, traced_per_world=a.traced, horizon=T, ticks=a.ticks,
                                  reps=a.reps, gpu=torch.cuda.get_device_name(0), commit=commit, median_ms=med, quartiles_ms=quart, launches=launches,
                                  host_waits=host_waits, equal=equal, reports_with_contacts=touched, reports=int(ref.shape[0] * ref.shape[1]),
                                  capacity_retries_in_timed_rounds=b.counter("capacity_retries") - retries0,
                                  actuators_skipped=b.counter("actuators_skipped"), device_skipped=b.counter("device_skipped"))), flush=True)
            del b, snap
    stream.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
