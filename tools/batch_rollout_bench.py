"""Times a horizon of T ticks under T control vectors with a trace of every tick, in the setting of tools/batch_actuator_bench.py - K
worlds of sphere_pile(8, 8, 8) after --ticks ticks, 64 actuators a world (16 bodies with four thrusters each, a clamp of [-1, 1] mN s),
16 traced bodies a world, impulse mode, one stream, wall clock from a synchronized stream to a completed synchronize, the two paths
alternating their order round by round, warm-up excluded, the median and the quartiles of --reps - two ways:
  (a) one rollout_dev;
  (b) the loop that defines it: actuate_dev(u[t]), step(dt, iters, 1), gather_state(row t), T times.
Every timed call starts from the same state: the batch is copied back from a snapshot batch (copy_worlds, unclocked) before it.
Before the timed rounds (a)'s traces and stats are compared with (b)'s from that state: equal bytes.  Run by hand; prints one JSON line
per K."""
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
    ap.add_argument("--bodies", type=int, default=16, help="actuated bodies a world")
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
            traced_np = (np.repeat(every, a.traced) * nb + np.tile(rng.choice(nb, a.traced, replace=False), K)).astype(np.int32)
            m = len(traced_np)
            d_u = torch.from_numpy(rng.uniform(-2e-3, 2e-3, (T, n)).astype(np.float32)).cuda()
            d_body = torch.from_numpy(traced_np).cuda()
            out = {p: {k: torch.empty((T, m, c), dtype=torch.float32, device="cuda") for k, c in (("x", 3), ("q", 4), ("v", 3), ("omega", 3))} for p in ("rollout", "loop")}
            stats = {}

            def sync():
                stream.synchronize()

            def reset():
                b.copy_worlds(every, snap, every)
                sync()

            def rollout():
                stats["rollout"] = bytes(b.rollout_dev(d_u, dt, iters, mgf_amd.ACTUATE_IMPULSE, body=d_body, **out["rollout"]))

            def loop():
                o, st = out["loop"], b""
                for t in range(T):
                    b.actuate_dev(d_u[t], mgf_amd.ACTUATE_IMPULSE)
                    st += bytes(b.step(dt, iters, 1))
                    b.gather_state(d_body, x=o["x"][t], q=o["q"][t], v=o["v"][t], omega=o["omega"][t])
                stats["loop"] = st

            # once, unclocked: (a) against (b) from the same state - traces, stats and the state the batch is left in
            end = {}
            for fn in (rollout, loop):
                reset()
                for o in out[fn.__name__].values():
                    o.fill_(float("nan"))
                fn()
                sync()
                end[fn.__name__] = b"".join(v.tobytes() for v in b.state().values())
            equal = dict(traces=all(out["rollout"][k].cpu().numpy().tobytes() == out["loop"][k].cpu().numpy().tobytes() for k in out["loop"]),
                         stats=stats["rollout"] == stats["loop"], state=end["rollout"] == end["loop"])
            retries0 = b.counter("capacity_retries")
            fns = (rollout, loop)
            t = {fn.__name__: [] for fn in fns}
            for rep in range(a.warmup + a.reps):
                for k in range(2):
                    fn = fns[(rep + k) % 2]
                    reset()
                    t0 = time.perf_counter()
                    fn()
                    sync()
                    if rep >= a.warmup:
                        t[fn.__name__].append(time.perf_counter() - t0)
            tick = b.counter("launches_per_tick")
            reset()
            rollout()
            launches = dict(rollout=T * tick + b.counter("rollout_launches"), loop=T * (tick + mgf_amd.BATCH_ACTUATOR_LAUNCHES + 1))
            sync()
            med = {k: round(1e3 * float(np.median(v)), 4) for k, v in t.items()}
            quart = {k: [round(1e3 * float(v_), 4) for v_ in np.percentile(v, [25, 75])] for k, v in t.items()}
            print(json.dumps(dict(K=K, bodies_per_world=nb, actuators_per_world=per, traced_per_world=a.traced, horizon=T, ticks=a.ticks, reps=a.reps,
                                  gpu=torch.cuda.get_device_name(0), commit=commit, median_ms=med, quartiles_ms=quart, launches=launches, equal=equal,
                                  rollout_launches=b.counter("rollout_launches"), capacity_retries_in_timed_rounds=b.counter("capacity_retries") - retries0,
                                  actuators_skipped=b.counter("actuators_skipped"), device_skipped=b.counter("device_skipped"))), flush=True)
            del b, snap
    stream.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
