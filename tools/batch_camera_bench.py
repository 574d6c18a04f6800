"""Times a depth image per world against the same rays as a sensor rig, in the setting of tools/batch_sensor_bench.py - K worlds of
sphere_pile(8, 8, 8) after --ticks ticks, one camera of --side x --side pixels and 90 degrees a world, --up above a sphere of the top
layer and looking down, the library's work on one stream, the paths rotating their order round by round, warm-up excluded, the median
and the quartiles of --reps rounds of --calls calls each - two ways:
  (a) cast_cameras_dev of a camera rig set once, depth only, mask ALL (k_batch_camera_tile: a workgroup per tile of 16 x 16 pixels);
  (b) cast_sensors_dev of a rig of one sensor a pixel, the same K * side * side rays (k_batch_sensor_ray): what a caller can do without
      cameras.
Also the host time of set_cameras against set_sensors for those rigs (the median of five).  Before the timed rounds the depth of (a) is
compared with the hits of (b) - the hit's t, or far - and with cast_cameras: equal bytes.
MGF_AMD_LIB names another build of the library, e.g. one of tools/build_variant.sh with -DMGF_CAMERA_CULL=0; "lib" in the output says
which was timed.  Run by hand; prints one JSON line per K."""
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
from mgf_amd import _capi, scenes  # noqa: E402


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def rotate(q, r):
    """Rotation::rotate_vector in f32, operation by operation"""
    s, v = q[:, 0:1], q[:, 1:4]
    return cross(v, cross(v, r) + r * s) * np.float32(2.0) + r


def pixel_dirs(width, height, tan_x, tan_y):
    f32 = np.float32
    ix, iy = np.arange(width, dtype=np.int64), np.arange(height, dtype=np.int64)
    u = ((2 * ix + 1).astype(f32) / f32(width) - f32(1.0)) * f32(tan_x)
    v = (f32(1.0) - (2 * iy + 1).astype(f32) / f32(height)) * f32(tan_y)
    d = np.empty((height, width, 3), f32)
    d[..., 0], d[..., 1], d[..., 2] = u[None, :], v[:, None], f32(1.0)
    return d.reshape(-1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[256])
    ap.add_argument("--side", type=int, default=64, help="pixels a side")
    ap.add_argument("--up", type=float, default=4.0, help="the eye above its body's centre, in the body's frame")
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--calls", type=int, default=10, help="calls a timed round")
    a = ap.parse_args()
    ctx = mgf_amd.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    sc = scenes.sphere_pile(8, 8, 8)
    dt, iters, nb = float(sc["dt"]), sc["iters"], len(sc["comps"])
    c = sc["comps"]["p"].astype(np.float64)
    top = np.flatnonzero(c[:, 1] > c[:, 1].max() - 0.5)
    body = int(top[np.argmin(np.sum(c[top][:, [0, 2]] ** 2, axis=1))])     # the sphere of the top layer nearest the middle
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
    except OSError:
        commit = ""
    s45 = float(np.sqrt(0.5))
    with torch.cuda.stream(stream):
        for K in a.ks:
            b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
            b.step(dt, iters, a.ticks)
            per = a.side * a.side
            n = K * per
            cams = np.zeros(K, _capi.CAMERA_DTYPE)
            cams["world"], cams["body"], cams["p"], cams["r"] = np.arange(K), body, (0.0, a.up, 0.0), (s45, s45, 0.0, 0.0)
            cams["tan_x"], cams["tan_y"], cams["far"], cams["width"], cams["height"], cams["flags"] = 1.0, 1.0, np.inf, a.side, a.side, 1
            dc = pixel_dirs(a.side, a.side, 1.0, 1.0)
            sens = np.zeros(n, _capi.SENSOR_DTYPE)
            sens["world"], sens["body"], sens["p"], sens["dt"], sens["flags"] = np.repeat(np.arange(K), per), body, (0.0, a.up, 0.0), np.inf, 1
            sens["d"] = np.tile(rotate(np.repeat(cams["r"][:1], per, axis=0), dc), (K, 1))
            set_ms = {"set_cameras": [], "set_sensors": []}
            for _ in range(5):
                t0 = time.perf_counter(); b.set_cameras(cams); set_ms["set_cameras"].append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter(); b.set_sensors(sens); set_ms["set_sensors"].append(1e3 * (time.perf_counter() - t0))
            depth = torch.empty(n, dtype=torch.float32, device="cuda")
            hits = torch.empty((n, 7), dtype=torch.int32, device="cuda")

            def sync():
                stream.synchronize()

            def cameras():
                b.cast_cameras_dev(depth=depth)

            def sensors():
                b.cast_sensors_dev(hits)

            sync()
            # once, unclocked: (a) against (b) and against the host-memory form
            depth.fill_(-1.0)
            cameras()
            sensors()
            sync()
            got = depth.cpu().numpy()
            h = hits.cpu().numpy().view(_capi.RAY_HIT_DTYPE).reshape(n)
            want = np.where(h["kind"] == -1, np.float32(np.inf), h["t"]).astype(np.float32)
            host = np.concatenate([im.ravel() for im in b.cast_cameras()])
            equal = dict(sensor_rig=got.tobytes() == want.tobytes(), cast_cameras=got.tobytes() == host.tobytes())
            kinds = {str(k): int(np.sum(h["kind"] == k)) for k in (-1, 0, 1, 2)}
            fns = (cameras, sensors)
            t = {fn.__name__: [] for fn in fns}
            for rep in range(a.warmup + a.reps):
                for k in range(2):
                    fn = fns[(rep + k) % 2]
                    sync()
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        fn()
                    sync()
                    if rep >= a.warmup:
                        t[fn.__name__].append((time.perf_counter() - t0) / a.calls)
            launches = {}
            for fn in fns:   # (unclocked)
                fn()
                launches[fn.__name__] = b.counter("query_launches")
            sync()
            med = {k: round(1e3 * float(np.median(v)), 4) for k, v in t.items()}
            quart = {k: [round(1e3 * float(q), 4) for q in np.percentile(v, [25, 75])] for k, v in t.items()}
            print(json.dumps(dict(K=K, bodies_per_world=nb, side=a.side, rays=n, ticks=a.ticks, reps=a.reps, calls=a.calls, gpu=torch.cuda.get_device_name(0),
                                  commit=commit, lib=os.environ.get("MGF_AMD_LIB", "libmgf_hip.so"), median_ms=med, quartiles_ms=quart, query_launches=launches,
                                  set_ms={k: round(float(np.median(v)), 3) for k, v in set_ms.items()}, kinds=kinds, equal=equal)), flush=True)
            del b
    stream.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
