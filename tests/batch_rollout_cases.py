"""Shared by the tests of a batch's rollouts (mgf_batch_rollout / _rollout_dev; WorldBatch.rollout / .rollout_dev), without a GPU: the
scenes and rig of tests/batch_actuator_cases.py with a row of controls per tick, and the scenes that make a capacity re-run happen in the
MIDDLE of a rollout - the late-contact pair: lattices of spheres with gaps between them and above the floor, every sphere moving towards
the lattice's foot, so that nothing touches for the first ticks and then everything does, with more constraints than a world's share
under cons_per_body = 1 holds - beside a sparse world that never outgrows its share.
tests/test_world_batch_rollout_host.py holds the scenes to the oracle."""
import numpy as np

from mgf_amd import _capi, scenes
from tests import batch_actuator_cases as AC

f32 = np.float32
IMPULSE, FORCE = AC.IMPULSE, AC.FORCE
T = 6                                # ticks of a rollout in the tests
LATE_A, LATE_B, SPARSE = range(3)    # the worlds of late_contact_scenes()
FIRST_CONTACT = 2                    # no world of the late-contact pair has a constraint before this tick


def closing_lattice(nx, ny, nz, gap, rate, name):
    """nx * ny * nz spheres r = 0.5 on a lattice of pitch 1 + gap whose lowest layer hangs `gap` above the floor of an open box, every
    sphere with the velocity -rate * (its centre - the foot of the lattice): all gaps close together, after about gap / ((1 + gap) rate)
    seconds"""
    pitch = 1.0 + gap
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    c = np.stack([(i.ravel() - (nx - 1) / 2.0) * pitch, 0.5 + gap + j.ravel() * pitch, (k.ravel() - (nz - 1) / 2.0) * pitch], axis=1).astype(f32)
    foot = f32([0.0, 0.5, 0.0])
    v0 = (-(c - foot) * f32(rate)).astype(f32)
    half = max(nx, nz) * pitch / 2.0 + 1.0
    return scenes._scene(name, scenes._spheres(c, 0.5), scenes.box_terrain(half, ny * pitch + 2.0, (0.0, 0.0, 0.0)), v0=v0)


def late_contact_scenes():
    """27 and 18 spheres that meet each other and the floor a few ticks in (the second a tick or so behind the first), and 8 spheres
    far apart that come to rest on the floor one by one"""
    late_a = closing_lattice(3, 3, 3, 0.30, 3.6, "closing_3x3x3")
    late_b = closing_lattice(3, 2, 3, 0.36, 3.4, "closing_3x2x3")
    i, k = np.meshgrid(np.arange(4), np.arange(2), indexing="ij")
    c = np.stack([(i.ravel() - 1.5) * 2.5 + 0.2, 0.52 + 0.05 * np.arange(8), (k.ravel() - 0.5) * 2.5 + 0.3], axis=1).astype(f32)
    sparse = scenes._scene("sparse_8", scenes._spheres(c, 0.5), scenes.box_terrain(7.0, 4.0, (0.0, 0.0, 0.0)), v0=np.zeros((8, 3), f32))
    return [late_a, late_b, sparse]


def share(n_bodies, cons_per_body=1):
    """the constraint records a world of n bodies starts with (batch_allot, host_batch.inc)"""
    return max(16, cons_per_body * n_bodies)


def late_rig(lengths, seed=151):
    """(rig, u, planted): 70 weak actuators over the three worlds in one seeded shuffle - every flag word, both clamps, a body with
    three of them - weak enough to leave the ticks of first contact where they are; one control is a NaN"""
    rng = np.random.default_rng(seed)
    counts = (30, 24, 16)
    world = np.concatenate([np.full(c, k, np.int32) for k, c in enumerate(counts)])
    body = np.concatenate([rng.integers(0, lengths[k], c) for k, c in enumerate(counts)]).astype(np.int32)
    body[:3] = 4
    order = rng.permutation(len(world))
    world, body = world[order], body[order]
    n = len(world)
    rig = np.zeros(n, _capi.ACTUATOR_DTYPE)
    rig["world"], rig["body"] = world, body
    rig["flags"] = np.arange(n) % 4
    rig["gain"] = rng.uniform(0.01, 0.05, n) * rng.choice([1.0, -1.0], n)
    rig["p"] = rng.uniform(-0.5, 0.5, (n, 3))
    d = rng.normal(0, 1, (n, 3))
    rig["d"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rig["lo"], rig["hi"] = -np.inf, np.inf
    clamp = rng.random(n) < 0.5
    rig["lo"][clamp], rig["hi"][clamp] = -0.5, 0.5
    u = rng.uniform(-1.0, 1.0, n).astype(f32)
    nan = int(np.flatnonzero(clamp)[3])
    u[nan] = np.nan
    return rig, u, [nan]


def controls(u, planted, ticks=T, seed=157):
    """[ticks, n] rows of controls from one: every row another scaling and another seeded offset of u, the planted non-finite
    controls as they are in every row"""
    rng = np.random.default_rng(seed)
    rows = np.stack([(u * f32(0.4 + 0.25 * t) + rng.uniform(-0.2, 0.2, len(u)).astype(f32)).astype(f32) for t in range(ticks)])
    rows[:, planted] = u[planted]
    assert rows.dtype == f32 and len({r.tobytes() for r in rows}) == ticks
    return np.ascontiguousarray(rows)


def traced(total, seed=163, count=40):
    """the traced bodies of a batch of `total` bodies: a shuffled subset with one index twice, and two indices outside the batch"""
    rng = np.random.default_rng(seed)
    body = rng.permutation(total)[:min(count, total)].astype(np.int32)
    body = np.concatenate([body, body[2:3], np.int32([total, -1])])
    body = body[rng.permutation(len(body))]
    return np.ascontiguousarray(body, np.int32), 2
