"""The oracle's pair candidates on the scenes of wide bodies that meet (tests/wide_pairs.py), counted again by brute force: every (i, j),
j < i, whose tight box of i meets the fat box of j (bvh.rs:297, world.rs:266) on the boxes of the oracle's own world BVH.  The GPU tests of
these scenes (test_gpu_wide_pairs.py) take the oracle as their ground truth; this pins what it accepts, on a machine without a GPU."""
import numpy as np
import pytest

from tests import wide_pairs as W
from tests.util import oracle_world

SINGLE = ("spheres", "capsules", "capsule_vs_sphere")  # worlds whose every body's tight box tight_boxes forms


def _check_ticks(sc, ticks, pair=None, meet=None, margin=0.0):
    ow = oracle_world(sc)
    dt, it = float(sc["dt"]), sc["iters"]
    single = np.ones(len(ow), bool)
    for s in range(ticks):
        n_cand = ow.build_constraints(dt).n_pair_candidates
        tc, tr = W.tight_boxes(ow)
        fc, fr = W.fat_boxes(ow)
        acc = W.accepted_pairs(tc, tr, fc, fr, single)
        assert len(acc) == n_cand, f"tick {s}: {len(acc)} pairs by brute force, the oracle counted {n_cand}"
        if s == meet:
            assert pair in acc, f"tick {s}: the runaways {pair} are not a candidate pair"
            W.lost_region_checks(ow, pair[0], pair[1], pair, margin)
        ow.solve(it)


@pytest.mark.parametrize("fast_larger", [True, False], ids=["fast_has_larger_id", "fast_has_smaller_id"])
@pytest.mark.parametrize("motion", ["head_on", "catch_up"])
@pytest.mark.parametrize("kind", SINGLE)
def test_oracle_accepts_the_meeting_runaways(kind, motion, fast_larger):
    sc, pair = W.meeting_scene(kind, motion, fast_larger)
    _check_ticks(sc, W.MEET_TICK + 2, pair, W.MEET_TICK, W.min_margin(kind))


@pytest.mark.parametrize("kind", ["two_part_bodies", "sixteen_part_bodies"])
@pytest.mark.parametrize("motion", ["head_on", "catch_up"])
def test_meeting_runaways_sit_in_the_lost_region(kind, motion):
    """the scenes of bodies of several parts: the runaways are plain spheres, the precondition of the GPU tests holds"""
    for fast_larger in (True, False):
        sc, (i, j) = W.meeting_scene(kind, motion, fast_larger)
        ow = oracle_world(sc)
        dt, it = float(sc["dt"]), sc["iters"]
        for s in range(W.MEET_TICK + 1):
            ow.build_constraints(dt)
            if s == W.MEET_TICK:
                W.lost_region_checks(ow, i, j, (i, j), W.min_margin(kind))
            ow.solve(it)


@pytest.mark.parametrize("seed", [0, 3, 7])
def test_oracle_counts_the_random_runaways_pairs(seed):
    sc, _ = W.fuzz_scene(seed, "spheres")
    _check_ticks(sc, 12)
