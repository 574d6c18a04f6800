"""Times a horizon of T ticks under T control vectors with a state trace AND the ray sensors' answers of every tick, in the setting of
tools/batch_rollout_bench.py - K worlds of sphere_pile(8, 8, 8) after --ticks ticks, 64 actuators a world (16 bodies with four
thrusters each, a clamp of [-1, 1] mN s), 64 ray sensors a world (16 bodies with four rays each, any way, every second one a segment,
all ignoring their own body), 16 traced bodies a world, impulse mode, mask QUERY_ALL, one stream, wall clock from a synchronized stream
to a completed synchronize, the paths rotating their order round by round, warm-up excluded, the median and the quartiles of --reps:
  (a) one rollout_observe_dev, hits (28 bytes an entry);
  (b) one rollout_observe_dev, depths (4 bytes);
  (c) the loop that defines it: actuate_dev(u[t]), step(dt, iters, 1), gather_state(row t), cast_sensors_dev(row t), T times;
  (d) rollout_dev alone: what the trace costs is (a) - (d);
  (e) one cast_sensors_dev on its own, to hold T of them against (a) - (d).
Every timed call starts from the same state: the batch is copied back from a snapshot batch (copy_worlds, unclocked) before it.
Before the timed rounds (a)'s rows, traces and stats are compared with (c)'s from that state: equal bytes; the depth rows are the hit's
t, or the sensor's dt where nothing is hit.  Run by hand; prints one JSON line per K."""
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
    ap.add_argument("--each", type=int, default=4, help="actuators a body, and rays a body")
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
            # the sensors: a.each rays on each of a.bodies bodies of every world, from the body's centre
            on = np.tile(np.repeat(rng.choice(nb, a.bodies, replace=False), a.each), K).astype(np.int32)
            s_d = rng.normal(0, 1, (n, 3))
            s_d = (s_d / np.linalg.norm(s_d, axis=1, keepdims=True)).astype(np.float32)
            s_dt = np.where(np.arange(n) % 2, 3.0, np.inf).astype(np.float32)
            b.set_sensors(world_np, on, p=np.zeros((n, 3), np.float32), d=s_d, dt=s_dt, ignore_self=True)
            ns = b.sensor_count()
            traced_np = (np.repeat(every, a.traced) * nb + np.tile(rng.choice(nb, a.traced, replace=False), K)).astype(np.int32)
            m = len(traced_np)
            d_u = torch.from_numpy(rng.uniform(-2e-3, 2e-3, (T, n)).astype(np.float32)).cuda()
            d_body = torch.from_numpy(traced_np).cuda()
            paths = ("observe_hit", "observe_depth", "loop", "rollout")
            out = {p: {k: torch.empty((T, m, c), dtype=torch.float32, device="cuda") for k, c in TRACES} for p in paths}
            rows = {"observe_hit": torch.empty((T, ns, 7), dtype=torch.int32, device="cuda"), "observe_depth": torch.empty((T, ns), dtype=torch.float32, device="cuda"),
                    "loop": torch.empty((T, ns, 7), dtype=torch.int32, device="cuda")}
            one = torch.empty((ns, 7), dtype=torch.int32, device="cuda")
            stats, extra = {}, {}

            def sync():
                stream.synchronize()

            def reset():
                b.copy_worlds(every, snap, every)
                sync()

            def observe_hit():
                stats["observe_hit"] = bytes(b.rollout_observe_dev(d_u, dt, iters, mgf_amd.ACTUATE_IMPULSE, body=d_body, sensors=rows["observe_hit"], **out["observe_hit"]))

            def observe_depth():
                stats["observe_depth"] = bytes(b.rollout_observe_dev(d_u, dt, iters, mgf_amd.ACTUATE_IMPULSE, body=d_body, sensors=rows["observe_depth"], depth=True,
                                                                     **out["observe_depth"]))

            def rollout():
                stats["rollout"] = bytes(b.rollout_dev(d_u, dt, iters, mgf_amd.ACTUATE_IMPULSE, body=d_body, **out["rollout"]))

            def loop():
                o, st = out["loop"], b""
                for t in range(T):
                    b.actuate_dev(d_u[t], mgf_amd.ACTUATE_IMPULSE)
                    st += bytes(b.step(dt, iters, 1))
                    b.gather_state(d_body, x=o["x"][t], q=o["q"][t], v=o["v"][t], omega=o["omega"][t])
                    b.cast_sensors_dev(rows["loop"][t])
                stats["loop"] = st

            def cast():
                b.cast_sensors_dev(one)

            fns = (observe_hit, observe_depth, loop, rollout)
            # once, unclocked: every path from the same state - sensor rows, traces, stats and the state the batch is left in
            end = {}
            for fn in fns:
                reset()
                for o in out[fn.__name__].values():
                    o.fill_(float("nan"))
                if fn.__name__ in rows:
                    rows[fn.__name__].view(torch.int32).fill_(0x5A5A5A5A)
                retries = b.counter("capacity_retries")
                fn()
                sync()
                extra[fn.__name__] = dict(rollout_launches=b.counter("rollout_launches"), passes=1 + b.counter("capacity_retries") - retries)
                end[fn.__name__] = b"".join(v.tobytes() for v in b.state().values())
            hit, depth, ref = (rows[p].cpu().numpy() for p in paths[:3])
            ref_t = np.ascontiguousarray(ref[:, :, 6]).view(np.float32)
            want_depth = np.where(ref[:, :, 0] == mgf_amd.HIT_NONE, s_dt[None, :], ref_t).astype(np.float32)
            equal = dict(observe_hit=hit.tobytes() == ref.tobytes(), observe_depth=depth.tobytes() == want_depth.tobytes(),
                         traces=all(out[p][k].cpu().numpy().tobytes() == out["loop"][k].cpu().numpy().tobytes() for p in paths for k, _ in TRACES),
                         stats=all(stats[p] == stats["loop"] for p in paths), state=all(end[p] == end["loop"] for p in paths))
            kinds = {str(k): int((ref[:, :, 0] == k).sum()) for k in (-1, 0, 1, 2)}
            retries0 = b.counter("capacity_retries")
            timed = fns + (cast,)
            t = {fn.__name__: [] for fn in timed}
            for rep in range(a.warmup + a.reps):
                for k in range(len(timed)):
                    fn = timed[(rep + k) % len(timed)]
                    reset()
                    if fn is cast:
                        b.cast_sensors_dev(one)   # (the collider gather behind the copy is not the cast's: it rides on this unclocked one)
                        sync()
                    t0 = time.perf_counter()
                    fn()
                    sync()
                    if rep >= a.warmup:
                        t[fn.__name__].append(time.perf_counter() - t0)
            tick = b.counter("launches_per_tick")
            launches = {p: T * tick + extra[p]["rollout_launches"] for p in ("observe_hit", "observe_depth", "rollout")}
            launches["loop"] = T * (tick + mgf_amd.BATCH_ACTUATOR_LAUNCHES + 1 + 2)   # (the cast behind a step: the gather and the body pass; no world has an obstacle)
            host_waits = {p: extra[p]["passes"] for p in ("observe_hit", "observe_depth", "rollout")}
            host_waits["loop"] = T
            med = {k: round(1e3 * float(np.median(v)), 4) for k, v in t.items()}
            quart = {k: [round(1e3 * float(v_), 4) for v_ in np.percentile(v, [25, 75])] for k, v in t.items()}
            print(json.dumps(dict(K=K, bodies_per_world=nb, actuators_per_world=per, sensors_per_world=ns // K, traced_per_world=a.traced, horizon=T, ticks=a.ticks,
                                  reps=a.reps, gpu=torch.cuda.get_device_name(0), commit=commit, median_ms=med, quartiles_ms=quart, launches=launches,
                                  host_waits=host_waits, equal=equal, kinds=kinds, trace_cost_ms=round(med["observe_hit"] - med["rollout"], 4),
                                  horizon_times_one_cast_ms=round(T * med["cast"], 4),
                                  capacity_retries_in_timed_rounds=b.counter("capacity_retries") - retries0,
                                  actuators_skipped=b.counter("actuators_skipped"), device_skipped=b.counter("device_skipped"))), flush=True)
            del b, snap
    stream.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
