"""Per-body contact summaries and box overlaps of a batch (mgf_batch_read_body_contacts, mgf_batch_overlap_aabb_many).
Contacts: every record of every answer bit-equal to the fold include/mgf_hip.h defines, computed in a numpy f32 loop
(tests/batch_observe_cases.fold) once over the oracle's constraint list of the same ticks and once over mgf_batch_read_constraints.
Overlaps: against Overlaps<AABB> over BoundedBy<AABB> of the colliders in numpy f32 (Targets.boxes of the lone world's query tests) and,
bit for bit, against the lone mgf_world that holds the same bodies and has been through the same calls."""
import numpy as np
import pytest

import mgf_amd
from mgf_amd import scenes
from tests import batch_observe_cases as OC
from tests import batch_query_cases as BQ
from tests.util import bits_equal, compare_constraints, oracle_world

pytestmark = pytest.mark.gpu
STATE = ("x", "q", "v", "omega", "delta")
ZERO = np.zeros(1, mgf_amd.BODY_CONTACTS_DTYPE)[0]


@pytest.fixture(scope="module")
def ctx():
    c = mgf_amd.Context(0)
    yield c
    c.close()


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_records(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(len(got)) if got[i:i + 1].tobytes() != want[i:i + 1].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} records differ, the first at body {bad[0]}: {got[bad[0]]} against {want[bad[0]]}")


def check_world(mine, n, oracle_cons, got, what):
    """a world's answer against the fold of the oracle's list and of the batch's own list `mine` of the same tick"""
    compare_constraints(mine, oracle_cons, check_impulse=True)
    same_records(got, OC.fold(oracle_cons, n), f"{what}: against the oracle's list")
    same_records(got, OC.fold(mine, n), f"{what}: against mgf_batch_read_constraints")


def snapshots(ctx, scs, ticks, iters=None, options=None):
    """the batch of `scs` beside one oracle world per scene; at each tick of `ticks`: (whole-batch answer, per-world answers, oracle lists,
    the batch's own lists)"""
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs)
    for key, v in (options or {}).items():
        b.set_option(key, v)
    ows = [oracle_world(sc) for sc in scs]
    dt = float(scs[0]["dt"])
    iters = scs[0]["iters"] if iters is None else iters
    out, at = {}, 0
    for t in ticks:
        b.step(dt, iters, t - at)
        for ow in ows:
            for _ in range(t - at):
                ow.step(dt, iters)
        at = t
        out[t] = (b.body_contacts(), [b.body_contacts(k) for k in range(len(scs))], [ow.constraints() for ow in ows],
                  [b.constraints(k) for k in range(len(scs))])
    return b, out


# ---- contacts 1: the piles ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def piles(ctx):
    scs = BQ.pile_scenes()
    b, snaps = snapshots(ctx, scs, (1, 2, 30))
    return dict(scs=scs, b=b, snaps=snaps)


@pytest.mark.parametrize("tick", [1, 2, 30])
def test_piles_every_world_and_the_whole_batch(ctx, piles, tick):
    scs = piles["scs"]
    whole, per_world, lists, mine = piles["snaps"][tick]
    assert [len(sc["comps"]) for sc in scs] == [1, 96, 512, 0, 1024]
    assert len(whole) == 1633
    same_records(whole, np.concatenate(per_world), "world = -1 is the worlds concatenated in order")
    for k, sc in enumerate(scs):
        check_world(mine[k], len(sc["comps"]), lists[k], per_world[k], f"tick {tick} world {k}")
    if tick == 30:
        assert OC.categories(lists[4], 1024) == (1856, 1020, 64, 770, 4) and len(lists[2]) == 952
    big = per_world[4]
    records, touching, terrain, as_b, free = OC.categories(lists[4], 1024)
    assert records > 0 and touching > 0 and terrain > 0 and as_b > 0 and free > 0
    assert int(np.sum(big["n_contacts"] > 0)) == touching and int(big["n_terrain"].sum()) == terrain and int(np.sum(big["n_contacts"] == 0)) == free
    assert int(big["n_contacts"].sum()) == 2 * records - terrain
    assert same_bytes(big[big["n_contacts"] == 0], np.repeat(ZERO, free))
    assert np.any(big["normal_impulse"] > 0) and np.any(big["impulse"] != 0)


# ---- contacts 2: the hub ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hub_first", [True, False], ids=["hub_is_b_300_times", "hub_own_range_of_300"])
def test_hub_a_chain_longer_than_a_workgroup(ctx, hub_first):
    sc, hub = OC.hub_scene(hub_first)
    b = mgf_amd.WorldBatch.from_scenes(ctx, [sc])
    ow = oracle_world(sc)
    dt, iters = float(sc["dt"]), sc["iters"]
    for tick in (1, 2):
        b.step(dt, iters)
        ow.step(dt, iters)
        cons = ow.constraints()
        got = b.body_contacts(0)
        check_world(b.constraints(0), 301, cons, got, f"hub tick {tick}")
        assert len(cons) == 300 and got["n_contacts"][hub] == 300 and np.all(np.delete(got["n_contacts"], hub) == 1)
        if tick == 1:
            assert 455.0 < got["normal_impulse"][hub] < 465.0
        same_records(b.body_contacts(), got, "world = -1 of a batch of one world")


# ---- contacts 3: capsules over a heightfield ---------------------------------------------------------------------------------------------
def test_capsules_over_a_heightfield(ctx):
    scs = OC.capsule_scenes()
    b, snaps = snapshots(ctx, scs, (20, 40))
    for tick, (whole, per_world, lists, mine) in snaps.items():
        same_records(whole, np.concatenate(per_world), f"tick {tick}: whole batch")
        for k, sc in enumerate(scs):
            check_world(mine[k], len(sc["comps"]), lists[k], per_world[k], f"tick {tick} world {k}")
            assert per_world[k]["n_terrain"].max() >= 2          # two contacts a face: two records of one body against the terrain
    assert all(np.sum(snaps[40][2][k]["b"] >= 0) > 0 for k in range(2))


# ---- contacts 4: iters = 0 ----------------------------------------------------------------------------------------------------------------
def test_no_solver_iterations_counts_without_impulses(ctx):
    scs = BQ.pile_scenes()[1:3]
    b, snaps = snapshots(ctx, scs, (3,), iters=0)
    whole, per_world, lists, mine = snaps[3]
    for k, sc in enumerate(scs):
        check_world(mine[k], len(sc["comps"]), lists[k], per_world[k], f"iters = 0 world {k}")
        assert per_world[k]["n_contacts"].sum() > 100 and per_world[k]["n_terrain"].sum() > 0
        for f in ("impulse", "normal_impulse"):
            assert not np.any(np.ascontiguousarray(per_world[k][f]).view(np.uint32)), f"{f} is not exactly +0"


# ---- contacts 5: empty and short cases ----------------------------------------------------------------------------------------------------
def test_before_a_tick_behind_added_bodies_and_a_short_buffer(ctx):
    scs = BQ.pile_scenes()
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs)
    assert same_bytes(b.body_contacts(), np.repeat(ZERO, 1633))           # before any tick
    assert len(b.body_contacts(3)) == 0                                   # the empty world
    b.step(float(scs[0]["dt"]), scs[0]["iters"], 2)
    assert len(b.body_contacts(3)) == 0 and b.body_contacts(2)["n_contacts"].sum() > 0
    lib = mgf_amd.load_library()
    buf = np.zeros(1633, mgf_amd.BODY_CONTACTS_DTYPE)
    for world, n in ((-1, 1633), (2, 512), (4, 1024)):
        assert lib.mgf_batch_read_body_contacts(b._h, world, buf.ctypes.data, n - 1) == mgf_amd._capi.ERR_CAPACITY
        assert lib.mgf_batch_read_body_contacts(b._h, world, buf.ctypes.data, n) == 0
    assert lib.mgf_batch_read_body_contacts(b._h, 3, buf.ctypes.data, 0) == 0
    for world in (5, 6, 1 << 33):
        assert lib.mgf_batch_read_body_contacts(b._h, world, buf.ctypes.data, 1633) == mgf_amd._capi.ERR_INVALID
        assert "world index" in lib.mgf_last_error().decode()
    # bodies added behind a tick: the lists of every world are empty until the next tick, as mgf_batch_read_constraints has them
    extra = scenes.sphere_pile(1, 1, 1)
    new = extra["comps"].copy()
    new["p"] += np.float32([0.0, 30.0, 0.0])
    b.add_bodies(0, new, extra["mass"], extra["restitution"], extra["friction"], extra["force"])
    assert all(len(b.constraints(k)) == 0 for k in range(5))
    assert same_bytes(b.body_contacts(), np.repeat(ZERO, 1634))
    b.step(float(scs[0]["dt"]), scs[0]["iters"])
    for k in (0, 2):
        same_records(b.body_contacts(k), OC.fold(b.constraints(k), b.world_len(k)), f"world {k} after the next tick")
    assert b.body_contacts(2)["n_contacts"].sum() > 0


# ---- contacts 6: a tick that was run again for capacity -----------------------------------------------------------------------------------
def test_a_tick_run_again_for_capacity(ctx):
    scs = BQ.pile_scenes()
    b, snaps = snapshots(ctx, scs, (12,), options=dict(cons_per_body=1))
    assert b.counter("capacity_retries") > 0
    whole, per_world, lists, mine = snaps[12]
    same_records(whole, np.concatenate(per_world), "whole batch")
    for k, sc in enumerate(scs):
        check_world(mine[k], len(sc["comps"]), lists[k], per_world[k], f"world {k} behind a capacity re-run")
    assert len(lists[2]) > 512


# ---- contacts 7: independence -------------------------------------------------------------------------------------------------------------
def test_an_answer_depends_on_its_world_only(ctx, piles):
    scs = piles["scs"]
    want = piles["snaps"][30][1]
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    rb = mgf_amd.WorldBatch.from_scenes(ctx, scs[::-1])
    rb.step(dt, iters, 30)
    same_records(rb.body_contacts(), np.concatenate(want[::-1]), "a batch built in reverse order")
    for k in (1, 2, 4):
        one = mgf_amd.WorldBatch.from_scenes(ctx, [scs[k]])
        one.step(dt, iters, 30)
        same_records(one.body_contacts(0), want[k], f"world {k} alone")
    many = mgf_amd.WorldBatch.from_scenes(ctx, [scs[1]] * 300)    # more worlds than compute units
    many.step(dt, iters, 30)
    same_records(many.body_contacts(), np.tile(want[1], 300), "300 copies of the 96-sphere world")
    same_records(many.body_contacts(299), want[1], "the last copy")


# ---- contacts 8, overlaps 5: the tick is untouched ----------------------------------------------------------------------------------------
def test_the_tick_is_untouched(ctx):
    scs = [scenes.sphere_pile(4, 6, 4, seed=5), scenes.capsule_field(3, 2, 3)]
    scs[1] = dict(scs[1], terrain=scs[0]["terrain"])
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    a, b = mgf_amd.WorldBatch.from_scenes(ctx, scs), mgf_amd.WorldBatch.from_scenes(ctx, scs)
    rng = np.random.default_rng(8)
    world = rng.integers(0, 2, 40).astype(np.int32)
    boxes = np.concatenate([rng.uniform(-3, 3, (40, 3)) + (0, 3, 0), rng.uniform(0.3, 2.0, (40, 3))], axis=1).astype(np.float32)
    contacts = hits = 0
    for _ in range(30):
        a.step(dt, iters)
        b.step(dt, iters)
        contacts += int(b.body_contacts()["n_contacts"].sum()) + int(b.body_contacts(1)["n_contacts"].sum())
        hits += len(b.overlap_boxes(world, boxes)[1])
    assert contacts > 0 and hits > 0
    assert a.counter("launches_per_tick") == b.counter("launches_per_tick") == 6
    for k in range(2):
        sa, sb = a.state(k), b.state(k)
        for f in STATE:
            assert bits_equal(sa[f], sb[f]), (k, f)
        ca, cb = a.constraints(k), b.constraints(k)
        assert same_bytes(ca, cb), f"world {k}: the constraint lists differ"
        same_records(a.body_contacts(k), b.body_contacts(k), f"world {k}")


# ---- contacts 9: write_state does not change the answer -----------------------------------------------------------------------------------
def test_unchanged_by_write_state_until_the_next_tick(ctx, piles):
    scs, b = piles["scs"], piles["b"]
    before = b.body_contacts()
    st = b.state(2)
    b.write_state(2, x=(st["x"] + np.float32([0.0, 5.0, 0.0])).astype(np.float32), v=np.zeros_like(st["v"]))
    same_records(b.body_contacts(), before, "after write_state of world 2")
    same_records(b.body_contacts(2), piles["snaps"][30][1][2], "world 2 itself")
    b.write_state(2, x=st["x"], v=st["v"])      # (the fixture's batch as the other tests expect it)


# ---- contacts 10, overlaps 5: the launch counter ------------------------------------------------------------------------------------------
def test_the_launch_count_does_not_grow_with_the_batch(ctx):
    sc = scenes.sphere_pile(2, 2, 2)
    counts = []
    for K in (2, 64):
        b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
        b.step(float(sc["dt"]), 4, 3)
        got = b.body_contacts()
        lc = b.counter("query_launches")
        assert len(got) == 8 * K and got["n_contacts"].sum() > 0 and b.counter("query_run_ns") > 0
        b.body_contacts(K - 1)
        l1 = b.counter("query_launches")
        world = (np.arange(10 * K) % K).astype(np.int32)
        boxes = np.tile(np.float32([0.0, 1.0, 0.0, 2.0, 2.0, 2.0]), (10 * K, 1))
        off, vals = b.overlap_boxes(world, boxes, cap=80 * K)      # (the gather behind the step, count, fill)
        lo_first = b.counter("query_launches")
        off, vals = b.overlap_boxes(world, boxes, cap=80 * K)
        lo = b.counter("query_launches")
        assert len(vals) == 80 * K and b.counter("query_run_ns") > 0
        counts.append((lc, l1, lo_first, lo))
    assert counts[0] == counts[1] and counts[0] == (1, 1, 3, 2), counts


# ---- overlaps 1: mixed queries ------------------------------------------------------------------------------------------------------------
def lone_twins(ctx, scs, ticks):
    lone = [mgf_amd.World.from_scene(ctx, sc) for sc in scs]
    for w, sc in zip(lone, scs):
        if ticks and len(w):
            w.step_many(float(scs[0]["dt"]), scs[0]["iters"], ticks)
    return lone


def check_overlaps(b, lone, world, boxes, off, vals, what):
    """the CSR answer against the numpy formula over the batch's colliders, and against the lone worlds' overlap_boxes"""
    assert len(off) == len(boxes) + 1 and off[0] == 0 and off[-1] == len(vals)
    bx = [OC.tight_boxes(b.colliders(k)) for k in range(b.n_worlds)]
    lens = []
    for i in range(len(boxes)):
        want = OC.overlaps(bx[world[i]], boxes[i])
        g = vals[off[i]:off[i + 1]]
        assert np.array_equal(g, want), f"{what}: box {i} of world {world[i]}: {g} against {want}"
        lens.append(len(want))
    for k, w in enumerate(lone):
        sel = np.nonzero(world == k)[0]
        if len(sel) == 0:
            continue
        loff, lvals = w.overlap_boxes(boxes[sel]) if len(w) else (np.zeros(len(sel) + 1, np.int64), np.zeros(0, np.uint32))
        mine = np.concatenate([vals[off[i]:off[i + 1]] for i in sel] + [np.zeros(0, np.uint32)])
        assert np.array_equal(np.diff(loff), np.diff(off)[sel]) and same_bytes(mine.astype(np.uint32), lvals), f"{what}: the lone world {k} answers otherwise"
    return np.array(lens)


@pytest.fixture(scope="module")
def pile_boxes(ctx):
    scs = BQ.pile_scenes()
    out = {}
    for ticks, counts in ((0, BQ.COUNTS_T0), (30, BQ.COUNTS_T30)):
        b = mgf_amd.WorldBatch.from_scenes(ctx, scs)
        if ticks:
            b.step(float(scs[0]["dt"]), scs[0]["iters"], ticks)
        lone = lone_twins(ctx, scs, ticks)
        world, boxes = OC.mixed_boxes([b.colliders(k)["p"] for k in range(len(scs))], counts)
        off, vals = b.overlap_boxes(world, boxes)
        out[ticks] = dict(scs=scs, b=b, lone=lone, world=world, boxes=boxes, off=off, vals=vals)
    return out


@pytest.mark.parametrize("ticks", [0, 30])
def test_piles_mixed_boxes(pile_boxes, ticks):
    c = pile_boxes[ticks]
    counts = BQ.COUNTS_T30 if ticks else BQ.COUNTS_T0
    assert np.bincount(c["world"], minlength=5).tolist() == list(counts) and set(BQ.COUNTS_T0) | set(BQ.COUNTS_T30) == {0, 1, 3, 64, 257, 300}
    for k in range(5):
        if len(c["lone"][k]):
            assert same_bytes(c["b"].colliders(k), c["lone"][k].colliders()), f"world {k}: colliders"
    lens = check_overlaps(c["b"], c["lone"], c["world"], c["boxes"], c["off"], c["vals"], f"tick {ticks}")
    # (on the lattice of tick 0 a box of half width 1.5 meets at most 4 x 4 x 4 spheres; the settled pile gives lists longer than a wave)
    assert np.sum(lens == 0) > 10 and np.sum(lens == 1) > 10 and (lens.max() > 64 if ticks else lens.max() == 64), (np.sum(lens == 0), np.sum(lens == 1), lens.max())


def test_capsule_scene_mixed_boxes(ctx):
    scs = OC.capsule_scenes()
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs)
    b.step(float(scs[0]["dt"]), scs[0]["iters"], 40)
    lone = lone_twins(ctx, scs, 40)
    cen = []
    for k in range(2):
        col = b.colliders(k)
        assert same_bytes(col, lone[k].colliders())
        cen.append(col["p"] + 0.5 * col["d"] * (col["tag"] == 1)[:, None])
    world, boxes = OC.mixed_boxes(cen, (64, 257))
    off, vals = b.overlap_boxes(world, boxes)
    lens = check_overlaps(b, lone, world, boxes, off, vals, "capsules")
    assert np.sum(lens == 0) > 0 and lens.max() >= 3
    # overlap_aabb hands the same boxes over as corners
    lo, hi = boxes[:, :3] - boxes[:, 3:], boxes[:, :3] + boxes[:, 3:]
    off2, vals2 = b.overlap_aabb(world, lo, hi)
    q = np.concatenate([(hi + lo) / np.float32(2), (hi - lo) / np.float32(2)], axis=1).astype(np.float32)
    check_overlaps(b, lone, world, q, off2, vals2, "capsules, by corners")


# ---- overlaps 2: special boxes ------------------------------------------------------------------------------------------------------------
def test_special_boxes(pile_boxes):
    c = pile_boxes[30]
    b, lone = c["b"], c["lone"]
    bx = OC.tight_boxes(b.colliders(4))
    sp = OC.special_boxes(bx)
    world = np.full(len(sp), 4, np.int32)
    off, vals = b.overlap_boxes(world, sp)
    hits = [vals[off[i]:off[i + 1]] for i in range(len(sp))]
    assert np.array_equal(hits[0], np.arange(1024)), "a box over the whole world: all 1024 bodies, in order across the waves"
    assert len(hits[1]) == 0, "a box far away"
    assert np.float32(abs(np.float32(bx[0, 0] - sp[2, 0]))) == np.float32(bx[0, 3] + sp[2, 3])
    assert 0 in hits[2], "a face that equals the body's: the test is <="
    assert 0 not in hits[3], "its nextafter neighbour"
    assert len(hits[4]) == 0, "a NaN box"
    assert 0 in hits[5], "a negative half extent answers as the single test does"
    check_overlaps(b, lone, world, sp, off, vals, "special boxes")
    # the covering box against every world at once, the empty one included
    w5 = np.arange(5, dtype=np.int32)
    cover = np.tile(np.float32([0, 10, 0, 50, 50, 50]), (5, 1))
    off, vals = b.overlap_boxes(w5, cover)
    assert np.diff(off).tolist() == [1, 96, 512, 0, 1024]
    assert np.array_equal(vals, np.concatenate([np.arange(n) for n in (1, 96, 512, 0, 1024)]))


# ---- overlaps 3: the capacity contract ----------------------------------------------------------------------------------------------------
def test_a_short_buffer_still_gets_offsets_and_total(pile_boxes):
    import ctypes as C
    c = pile_boxes[30]
    b, world, boxes, off = c["b"], c["world"], c["boxes"], c["off"]
    total = len(c["vals"])
    lib = mgf_amd.load_library()
    wd = np.ascontiguousarray(world)
    for cap in (total - 1, 0):
        o = np.full(len(boxes) + 1, 7, np.uint64)
        v = np.zeros(total, np.uint32)
        t = C.c_int64(-5)
        st = lib.mgf_batch_overlap_aabb_many(b._h, wd.ctypes.data, boxes.ctypes.data, len(boxes), o.ctypes.data, v.ctypes.data, cap, C.byref(t))
        assert st == mgf_amd._capi.ERR_CAPACITY and t.value == total and np.array_equal(o.astype(np.int64), off), cap
    o = np.zeros(len(boxes) + 1, np.uint64)
    v = np.zeros(total, np.uint32)
    assert lib.mgf_batch_overlap_aabb_many(b._h, wd.ctypes.data, boxes.ctypes.data, len(boxes), o.ctypes.data, v.ctypes.data, total, None) == 0   # (total may be NULL)
    assert np.array_equal(v, c["vals"])
    with pytest.raises(mgf_amd.MgfError) as e:
        b.overlap_boxes(np.int32([0, 5]), boxes[:2])
    assert e.value.status == mgf_amd._capi.ERR_INVALID and "world index" in str(e.value)


# ---- overlaps 4: independence -------------------------------------------------------------------------------------------------------------
def test_a_list_depends_on_its_box_and_its_world_only(ctx, pile_boxes):
    c = pile_boxes[30]
    scs, b, world, boxes, off, vals = c["scs"], c["b"], c["world"], c["boxes"], c["off"], c["vals"]
    lists = [vals[off[i]:off[i + 1]] for i in range(len(boxes))]
    for i in range(0, len(boxes), 9):     # alone
        o, v = b.overlap_boxes(world[i:i + 1], boxes[i:i + 1])
        assert o.tolist() == [0, len(lists[i])] and np.array_equal(v, lists[i]), i
    r = slice(None, None, -1)             # the whole set in reversed order
    o, v = b.overlap_boxes(world[r], boxes[r])
    assert np.array_equal(np.diff(o), np.diff(off)[r]) and np.array_equal(v, np.concatenate(lists[::-1]))
    K = len(scs)                          # the same worlds in a batch built in reverse order
    rb = mgf_amd.WorldBatch.from_scenes(ctx, scs[::-1])
    rb.step(float(scs[0]["dt"]), scs[0]["iters"], 30)
    o, v = rb.overlap_boxes(K - 1 - world, boxes)
    assert np.array_equal(o, off) and np.array_equal(v, vals)


# ---- overlaps 5: edges --------------------------------------------------------------------------------------------------------------------
def test_no_boxes_is_a_valid_call(ctx):
    sc = scenes.sphere_pile(2, 2, 2)
    b = mgf_amd.WorldBatch.from_scenes(ctx, [sc, BQ.empty_scene(None)])
    off, vals = b.overlap_boxes(np.zeros(0, np.int32), np.zeros((0, 6), np.float32))
    assert off.tolist() == [0] and len(vals) == 0 and b.counter("query_launches") == 0
    off, vals = b.overlap_boxes(np.int32([1, 0, 1]), np.tile(np.float32([0, 1, 0, 9, 9, 9]), (3, 1)))     # the empty world
    assert off.tolist() == [0, 0, 8, 8] and vals.tolist() == list(range(8))
