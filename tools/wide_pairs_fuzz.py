"""Random runaways against the oracle, many seeds in one go (the suite runs 15 of them: tests/test_gpu_wide_pairs.py): 2..40 spheres of a
12^3 pile (even seeds) or of a small field of two-part bodies (odd seeds) thrown at 50..600 m/s from a shell outside the bounds or from inside,
a third of them aimed at another runaway; 36 ticks each of the list-on world, the list-off world and the oracle, bit for bit.

A seed where both GPU worlds agree with each other but not with the oracle's pair count is checked once more on the CPU: if the brute-force
predicate on the oracle's own leaf boxes counts what the GPU counted, the oracle's tree walk skipped a pair whose boxes touch exactly (an
internal node's centre / half-extent form rounds the touching case away) - reported apart, as it is no matter of the wide list.
python tools/wide_pairs_fuzz.py <first seed> <last seed>"""
import os, re, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import mgf_amd
from tests import wide_pairs as W
from tests.test_gpu_wide_pairs import _three_way
from tests.util import oracle_world


def leaf_count(sc, tick):
    """the oracle's pair count and the brute-force count on its leaf boxes in `tick`"""
    ow = oracle_world(sc)
    dt, it = float(sc["dt"]), sc["iters"]
    for _ in range(tick):
        ow.build_constraints(dt); ow.solve(it)
    n = ow.build_constraints(dt).n_pair_candidates
    tc, tr = W.tight_boxes(ow)
    fc, fr = W.fat_boxes(ow)
    return n, len(W.accepted_pairs(tc, tr, fc, fr, np.ones(len(ow), bool)))


ctx = mgf_amd.Context(0)
a, b = int(sys.argv[1]), int(sys.argv[2])
bad, touching, listed = [], [], 0
for seed in range(a, b):
    base = "spheres" if seed % 2 == 0 else "two_part_bodies"
    sc, bodies = W.fuzz_scene(W.FUZZ_SEED_BASE + seed, base)
    try:
        w, peak = _three_way(ctx, sc, 36, full_every=4)
        listed += w.counter("wide_ticks") > 0
        print(f"seed {seed}: {base} runaways {len(bodies)} wide ticks {w.counter('wide_ticks')} peak listed {peak} overflows {w.counter('wide_overflows')}: "
              "bit-identical", flush=True)
    except AssertionError as e:
        m = re.match(r"tick (\d+): list on and off \((\d+), \d+\), oracle \((\d+), \d+\)", str(e))
        if m and base == "spheres":
            tick, gpu = int(m.group(1)), int(m.group(2))
            ora, leaf = leaf_count(sc, tick)
            if leaf == gpu and ora == int(m.group(3)):
                touching.append(seed)
                print(f"seed {seed}: {base} runaways {len(bodies)}: tick {tick}: the GPU's {gpu} pairs are the leaf predicate's {leaf}, the oracle's tree "
                      f"walk found {ora} (exactly touching boxes)", flush=True)
                continue
        bad.append(seed)
        print(f"seed {seed}: {base} runaways {len(bodies)}: MISMATCH {e}", flush=True)
ctx.close()
print(f"{b - a} seeds, {listed} with ticks on the list, {len(bad)} mismatches {bad}, {len(touching)} exactly touching pairs the oracle's tree skips {touching}")
sys.exit(1 if bad else 0)
