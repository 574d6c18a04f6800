"""Times one iteration of a "touched by whom" observation on a batch whose answer is consumed on the device, in the setting and by the
method of tools/batch_zone_bench.py - K worlds of sphere_pile(8, 8, 8) after --ticks ticks, 64 contact sensors a world (16 bodies x
{MGF_TOUCH_ANY, _STATIC, _ANY_BODY, one partner taken from the body's own chain}), the library's work and torch's on one stream, the
paths rotating their order round by round, warm-up excluded, the median and the quartiles of --reps - three ways:
  (a) read_touches_dev of a rig set once, and a torch reduction of the reports (per world the contacts, the summed normal impulse and the
      strongest impulse its sensors report);
  (b) the answer as a caller gets it without the rig: constraints(k) for every world - a download and a host wait each - a vectorised
      numpy filter and sum per world (sensor x record masks, one matrix product for the impulses), the result copied to the device, the
      same reduction;
  (c) body_contacts_dev of the whole batch and a reduction of its records.  It does not answer the question - it has no partner - and
      is here as the cost of an unfiltered fold over the same lists.
(b) sums in numpy's order, so its floats agree with (a)'s to rounding only; (a) is held to its definition instead: before the timed
rounds its reports must equal the sequential fold (tests/batch_touch_cases.fold_touch) of (b)'s own lists byte for byte, and the
host-memory form's.  Run by hand; prints one JSON line per K."""
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
from tests import batch_touch_cases as TC  # noqa: E402

ANY, ANY_BODY, STATIC = mgf_amd.TOUCH_ANY, mgf_amd.TOUCH_ANY_BODY, mgf_amd.TOUCH_STATIC


def filtered(cons, body, other):
    """per sensor (n_contacts, impulse.xyz, normal_impulse) of one world's list, vectorised: numpy's sums, not the definition's order"""
    a, b, ni = cons["a"][None, :], cons["b"][None, :], cons["normal_impulse"].astype(np.float32)
    x, o = body[:, None], other[:, None]

    def match(partner):
        return np.where(o >= 0, partner == o, np.where(o == STATIC, partner < 0, np.where(o == ANY_BODY, partner >= 0, True)))
    as_a = ((a == x) & match(b)).astype(np.float32)
    as_b = ((b == x) & match(a)).astype(np.float32)
    t = cons["normal"].astype(np.float32) * ni[:, None]
    out = np.empty((len(body), 5), np.float32)
    out[:, 0] = as_a.sum(axis=1) + as_b.sum(axis=1)
    out[:, 1:4] = (as_b - as_a) @ t
    out[:, 4] = (as_a + as_b) @ ni
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[256], help="worlds")
    ap.add_argument("--bodies", type=int, default=16, help="bodies a world that carry sensors, four sensors each")
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--commit", default=None, help="the commit the JSON line names (default: git rev-parse --short HEAD)")
    a = ap.parse_args()
    ctx = mgf_amd.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    sc = scenes.sphere_pile(8, 8, 8)
    dt, iters, nb = float(sc["dt"]), sc["iters"], len(sc["comps"])
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], capture_output=True, text=True, cwd=os.path.dirname(os.path.abspath(__file__))).stdout.strip()
        except OSError:
            commit = ""
    with torch.cuda.stream(stream):
        for K in a.ks:
            b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
            b.step(dt, iters, a.ticks)
            first = b.constraints(0)                                    # (every world is the same scene: one list chooses the partners)
            rng = np.random.default_rng(2)
            bodies = np.sort(rng.choice(nb, a.bodies, replace=False))
            rows = []
            for x in bodies.tolist():
                ch = TC.chain(first, x, ANY_BODY)
                partner = ch[0][2] if ch else (x + 1) % nb
                rows += [(0, x, ANY, 0), (0, x, STATIC, 0), (0, x, ANY_BODY, 0), (0, x, partner, 0)]
            one = np.array(rows, mgf_amd.TOUCH_DTYPE)
            per, n = len(one), K * len(one)
            rig = np.tile(one, K)
            rig["world"] = np.repeat(np.arange(K, dtype=np.int32), per)
            b.set_touches(rig)
            out_a = torch.empty((n, 16), dtype=torch.float32, device="cuda")
            out_c = torch.empty((K * nb, 6), dtype=torch.float32, device="cuda")
            result = {}

            def sync():
                stream.synchronize()

            def reduce(count, nsum, strongest, key):
                result[key] = (count.view(K, -1).sum(dim=1), nsum.view(K, -1).sum(dim=1), strongest.view(K, -1).max(dim=1).values)

            def touches():
                b.read_touches_dev(out_a)
                reduce(out_a[:, 0].view(torch.int32), out_a[:, 7], out_a[:, 11], "touches")

            def lists():
                host = np.empty((n, 5), np.float32)
                for k in range(K):
                    host[k * per:(k + 1) * per] = filtered(b.constraints(k), one["body"], one["other"])
                d = torch.from_numpy(host).cuda()
                result["reports"] = d
                reduce(d[:, 0].to(torch.int32), d[:, 4], d[:, 4], "lists")                     # (no strongest record: the sum stands in)

            def unfiltered():
                b.body_contacts_dev(out_c)
                reduce(out_c[:, 0].view(torch.int32), out_c[:, 5], out_c[:, 5], "unfiltered")

            sync()
            # once, unclocked: (a) against the host-memory form, and against the sequential fold of (b)'s own lists
            out_a.view(torch.int32).fill_(0x5A5A5A5A)
            b.read_touches_dev(out_a)
            sync()
            got = out_a.cpu().numpy()
            own = {k: b.constraints(k) for k in range(K)}
            qs = {k: b.state(k)["q"] for k in range(K)}
            want = TC.fold_rig(rig, own, qs)
            equal = dict(read_touches=got.tobytes() == b.read_touches().tobytes(), fold_of_the_lists=got.tobytes() == want.tobytes())
            counts_b = np.concatenate([filtered(own[k], one["body"], one["other"])[:, 0] for k in range(K)])
            equal["counts_of_b"] = bool(np.array_equal(counts_b.astype(np.int64), want["n_contacts"]))
            fns = (touches, lists, unfiltered)
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
            for fn in (touches, unfiltered):   # (unclocked)
                fn()
                launches[fn.__name__] = b.counter("query_launches")
            sync()
            med = {key: round(1e3 * float(np.median(v)), 4) for key, v in t.items()}
            quart = {key: [round(1e3 * float(q), 4) for q in np.percentile(v, [25, 75])] for key, v in t.items()}
            print(json.dumps(dict(K=K, bodies_per_world=nb, sensors_per_world=per, records_per_world=len(first), ticks=a.ticks, reps=a.reps,
                                  gpu=torch.cuda.get_device_name(0), commit=commit, median_ms=med, quartiles_ms=quart, query_launches=launches,
                                  contacts_reported=int(result["touches"][0].sum().item()), contacts_of_the_lists=int(result["lists"][0].sum().item()),
                                  sensors_without_a_match=int(np.sum(want["n_contacts"] == 0)), equal=equal)), flush=True)
            del b
    stream.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
