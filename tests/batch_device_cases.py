"""Shared inputs of the tests of a batch's device-pointer calls (mgf_batch_gather_state_dev / _set_many_dev / _set_forces_dev /
_apply_impulses_dev / _read_body_contacts_dev / _copy_worlds_where): test_world_batch_device_host.py checks without a GPU that they
are not trivial, test_gpu_world_batch_device.py runs them on twin batches."""
import numpy as np

from mgf_amd import scenes

BLOCK = 256          # kBatchBlock: lanes of a workgroup of the per-record and per-body kernels
N_RECORDS = 600      # more than two blocks of records
N_DISTINCT = 200     # ... over about this many bodies
TRIPLE_AT = (10, 300, 590)   # the records that name one body three times, one in each block of records
TICKS = 3
QUIET_WORLD = 1      # the one-body world in the middle: no record of the setters' tests names it


def device_scenes():
    """three worlds of 5, 1 and 300 spheres, each over its own small box: the world of 300 lies across two 256-lane blocks of a
    kernel with a lane per body, and a world of one body sits between the two others"""
    return [scenes.sphere_pile(5, 1, 1, seed=201), scenes.sphere_pile(1, 1, 1, seed=202), scenes.sphere_pile(10, 3, 10, seed=203)]


def offsets(scs):
    return np.concatenate([[0], np.cumsum([len(sc["comps"]) for sc in scs])]).astype(np.int64)


def world_body(scs, flat):
    """the (world, body) pairs of flat indices: what the host-memory calls of twin A take"""
    off = offsets(scs)
    world = (np.searchsorted(off, flat, side="right") - 1).astype(np.int32)
    return world, (np.asarray(flat) - off[world]).astype(np.int32)


def triple_body(scs):
    """the body named three times: one of the world of 300, beyond the first block of bodies"""
    return int(offsets(scs)[2]) + 277


def records(scs, seed=31):
    """N_RECORDS flat body indices over N_DISTINCT bodies, none of QUIET_WORLD; triple_body() at TRIPLE_AT and nowhere else"""
    rng = np.random.default_rng(seed)
    off = offsets(scs)
    total, g3 = int(off[-1]), triple_body(scs)
    quiet = set(range(int(off[QUIET_WORLD]), int(off[QUIET_WORLD + 1])))
    pool = np.array([g for g in range(total) if g not in quiet and g != g3])
    chosen = rng.choice(pool, N_DISTINCT - 1, replace=False)
    flat = np.concatenate([chosen, rng.choice(chosen, N_RECORDS - len(chosen))])   # every chosen body at least once
    flat = flat[rng.permutation(N_RECORDS)]
    flat[list(TRIPLE_AT)] = g3
    return flat.astype(np.int32)


def rows(n, seed, scale):
    return np.random.default_rng(seed).uniform(-scale, scale, (n, 3)).astype(np.float32)


def impulse_rows(scs, seed=37):
    """(linear, angular) for records(): the triple's rows are 1e8, 1, -1e8 - in f32 (1e8 + 1) - 1e8 = 0 and (1e8 - 1e8) + 1 = 1: the
    sum depends on the order, so only the ascending record order gives the host path's answer"""
    lin, ang = rows(N_RECORDS, seed, 1.5), rows(N_RECORDS, seed + 1, 2.0)
    for at, val in zip(TRIPLE_AT, (1e8, 1.0, -1e8)):
        lin[at] = np.float32([val, -val, val])
        ang[at] = np.float32([val, val, -val])
    return lin, ang


def subset_with_repeats(scs, seed=41):
    """the gather's shuffled subset: 400 indices over all three worlds, bodies named again"""
    rng = np.random.default_rng(seed)
    total = int(offsets(scs)[-1])
    some = rng.choice(total, 150, replace=False)
    flat = np.concatenate([some, rng.choice(some, 250), [0, total - 1, int(offsets(scs)[QUIET_WORLD])]])
    return flat[rng.permutation(len(flat))].astype(np.int32)


# the masked copy: pairs in an order that puts the world of 300 - the one whose share must grow - in the middle, where mask [1, 0, 1] leaves it out
COPY_PAIRS = np.int32([0, 2, 1])
MASKS = ([1, 0, 1], [0, 0, 0], [1, 1, 1])
