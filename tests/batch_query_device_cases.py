"""The world arrays of tests/test_gpu_world_batch_query_device.py (mgf_batch_raycast_many_dev / _sweep_many_dev), shared with the CPU
check of the plan the device builds from them (tests/test_world_batch_query_device_host.py): the rays of the pile (tests 1 and 2), the
same rays with records the call must skip among them (test 4), and the batch of 300 one-sphere worlds (test 6) - and a numpy model of
that plan: counts, starts, work items of up to 256 queries, order."""
import numpy as np

from tests import batch_obstacle_cases as BC
from tests import batch_query_cases as BQ

PILE_BODIES = (1, 96, 512, 0, 1024)      # BQ.pile_scenes()
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
MANY = 300                                # worlds of test 6: more than a block of 256 plan lanes
TICKS = 30
# the world of 96 spheres has an obstacle list: a ring of ten spheres just above its pile (the pile's top sphere ends at y = 5.66, the
# ring begins at 5.95: the tick never meets it), in the way of rays that come from above
OBSTACLE_WORLD = 1
RING = (BC.compounds()["ring"], (0.0, 6.0, 0.0), BC.IDENT)
# and the world without bodies the same ring on the floor, for casts to come down on
EMPTY_WORLD = 3
LOW_RING = (BC.compounds()["ring"], (0.1, 0.05, -0.1), BC.IDENT)


def pile_scenes():
    scs = BQ.pile_scenes()
    scs[OBSTACLE_WORLD] = dict(scs[OBSTACLE_WORLD], obstacles=[RING])
    scs[EMPTY_WORLD] = dict(scs[EMPTY_WORLD], obstacles=[LOW_RING])
    return scs


def empty_world_casts():
    """the casts of the world without bodies: a sphere and a capsule straight down onto spheres of its ring, a sphere and a capsule
    straight down onto the floor beside it"""
    from mgf_amd._capi import MOVING_DTYPE
    ring = BC.component_centres([LOW_RING])
    c = np.zeros(4, MOVING_DTYPE)
    c["tag"] = [0, 1, 0, 1]
    c["r"] = [0.3, 0.25, 0.3, 0.3]
    c["d"] = [(0, 0, 0), (0.4, 0.0, 0.1), (0, 0, 0), (0.2, 0.0, 0.3)]
    c["p"] = [ring[1] + (0.0, 4.0, 0.0), ring[5] + (-0.2, 5.0, 0.0), (0.5, 2.0, 0.3), (-0.5, 2.0, -0.3)]
    c["delta"] = [(0, -6.0, 0), (0, -7.0, 0), (0, -4.0, 0), (0, -4.0, 0)]
    return c


def bad_worlds(n_worlds):
    """what a call skips: just below, just above, and the two ends of int32"""
    return np.array([-1, n_worlds, I32_MIN, I32_MAX], np.int32)


def pile_world_array():
    """world[] of BQ.pile_rays(..., COUNTS_T30): it depends on the number of centres a world has, not on where they are"""
    return BQ.pile_rays([np.zeros((c, 3)) for c in PILE_BODIES], BQ.COUNTS_T30)["world"]


def skip_positions(n, count, seed=77):
    """where the records to skip go among n + count records: the first, the last, and a seeded choice between"""
    rng = np.random.default_rng(seed)
    at = np.concatenate([[0, n + count - 1], 1 + rng.choice(n + count - 2, count - 2, replace=False)])
    return np.sort(at)


def spread(arrays, fill, at):
    """every array of `arrays` (n rows) with the rows of `fill` (len(at) rows, cycled) put in at the positions `at` of the result"""
    n = len(next(iter(arrays.values()))) + len(at)
    keep = np.ones(n, bool)
    keep[at] = False
    out = {}
    for k, a in arrays.items():
        r = np.empty((n,) + a.shape[1:], a.dtype)
        r[keep] = a
        r[at] = np.resize(fill[k], (len(at),) + a.shape[1:])
        out[k] = r
    return out, keep


def many_world_arrays():
    """test 6: one ray to each of MANY worlds in a shuffled order; MANY rays all to the last world"""
    return np.random.default_rng(6).permutation(MANY).astype(np.int32), np.full(MANY, MANY - 1, np.int32)


def plan_model(world, n_worlds):
    """the plan in numpy, by the steps of the device's kernels: a valid query counts itself into its world and keeps its rank (here: in
    array order - on the device in whatever order the lanes come), the counts and the item counts ceil(c / 256) are summed up, the query
    of rank r goes to order[start + r], and the one whose rank is a multiple of 256 writes the work item (world, first, count <= 256).
    Returns (items [m, 3], order [valid], skipped)."""
    world = np.asarray(world, np.int64)
    valid = (world >= 0) & (world < n_worlds)
    cnt = np.bincount(world[valid], minlength=n_worlds)
    start = np.concatenate([[0], np.cumsum(cnt)])
    istart = np.concatenate([[0], np.cumsum((cnt + 255) // 256)])
    rank = np.zeros(len(world), np.int64)
    seen = np.zeros(n_worlds, np.int64)
    for i in np.flatnonzero(valid):
        rank[i] = seen[world[i]]
        seen[world[i]] += 1
    order = np.full(int(start[-1]), -1, np.int64)
    items = np.full((int(istart[-1]), 3), -1, np.int64)
    for i in np.flatnonzero(valid):
        w, r = world[i], rank[i]
        order[start[w] + r] = i
        if r % 256 == 0:
            items[istart[w] + r // 256] = (w, start[w] + r, min(256, cnt[w] - r))
    return items, order, int(np.sum(~valid))
