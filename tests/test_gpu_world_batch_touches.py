"""Contact sensors of a batch (mgf_batch_set_touches, mgf_batch_read_touches, mgf_batch_read_touches_dev): every report byte for byte the
fold include/mgf_hip.h defines ("contact sensors"), computed in a numpy f32 loop (tests/batch_touch_cases.fold_touch) twice - over the
oracle's constraint list of the same tick and over mgf_batch_read_constraints - with q as mgf_batch_read_state returns it."""
import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi, scenes
from tests import batch_obstacle_cases as BC
from tests import batch_observe_cases as OC
from tests import batch_parts_cases as PC
from tests import batch_query_cases as BQ
from tests import batch_touch_cases as TC
from tests.util import bits_equal, compare_constraints, oracle_world

pytestmark = pytest.mark.gpu
STATE = ("x", "q", "v", "omega", "delta")
ANY, ANY_BODY, STATIC, NONE, FRAME = mgf_amd.TOUCH_ANY, mgf_amd.TOUCH_ANY_BODY, mgf_amd.TOUCH_STATIC, mgf_amd.TOUCH_NONE, mgf_amd.TOUCH_BODY_FRAME
FILL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    c = mgf_amd.Context(0)
    yield c
    c.close()


def no_match(n):
    out = np.zeros(n, mgf_amd.TOUCH_REPORT_DTYPE)
    out["partner"], out["record"] = NONE, -1
    return out


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def same_records(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = [i for i in range(len(got)) if got[i:i + 1].tobytes() != want[i:i + 1].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} of {len(got)} reports differ, the first at sensor {bad[0]}: {got[bad[0]]} against {want[bad[0]]}")


def worlds_of(rig):
    return sorted(set(rig["world"].tolist()))


def check(b, rig, oracle_lists, what):
    """the rig's reports against the fold of the oracle's lists and of the batch's own lists of the same tick; -> (reports, own lists, q)"""
    b.set_touches(rig)
    assert b.touch_count() == len(rig)
    got = b.read_touches()
    mine = {k: b.constraints(k) for k in worlds_of(rig)}
    qs = {k: b.state(k)["q"] for k in worlds_of(rig)}
    for k in mine:
        compare_constraints(mine[k], oracle_lists[k], check_impulse=True)
    same_records(got, TC.fold_rig(rig, oracle_lists, qs), f"{what}: against the oracle's list")
    same_records(got, TC.fold_rig(rig, mine, qs), f"{what}: against mgf_batch_read_constraints")
    assert not got["reserved0"].any() and not got["reserved1"].view(np.uint32).any()
    return got, mine, qs


def run_beside_oracle(ctx, scs, ticks, ows=None, iters=None, options=None, own_terrain=False):
    """the batch of `scs` beside one oracle world per scene, brought to each tick of `ticks` in turn: yields (tick, batch, the oracle's lists)"""
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=own_terrain)
    for key, v in (options or {}).items():
        b.set_option(key, v)
    ows = [oracle_world(sc) for sc in scs] if ows is None else ows
    dt = float(scs[0]["dt"])
    iters = scs[0]["iters"] if iters is None else iters
    at = 0
    for t in ticks:
        b.step(dt, iters, t - at)
        for ow in ows:
            for _ in range(t - at):
                ow.step(dt, iters)
        at = t
        yield t, b, [ow.constraints() for ow in ows]


def lengths_of(scs):
    return [PC.n_bodies(sc) for sc in scs]


# ---- 1: the piles -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def piles(ctx):
    scs = BQ.pile_scenes()
    lengths = lengths_of(scs)
    assert lengths == [1, 96, 512, 0, 1024]
    snaps, b = {}, None
    for t, b, lists in run_beside_oracle(ctx, scs, TC.PILE_TICKS):
        rig = TC.rig_of(lists, lengths, skip=(TC.NO_SENSOR_WORLD,))
        got, mine, qs = check(b, rig, lists, f"tick {t}")
        snaps[t] = dict(rig=rig, got=got, lists=lists, mine=mine, qs=qs, contacts=[b.body_contacts(k) for k in range(len(scs))])
    return dict(scs=scs, lengths=lengths, b=b, snaps=snaps)


@pytest.mark.parametrize("tick", TC.PILE_TICKS)
def test_piles_every_filter_in_shuffled_world_order(piles, tick):
    s = piles["snaps"][tick]
    rig, got = s["rig"], s["got"]
    assert worlds_of(rig) == [1, 2, 4] and np.any(np.diff(rig["world"]) < 0) and len(rig) > 150      # no sensor on world 0, world 3 unnamed, mixed order
    for i, r in enumerate(rig):
        bc = s["contacts"][int(r["world"])][int(r["body"])]
        if r["other"] == ANY and not r["flags"]:
            assert (got[i]["n_contacts"], got[i]["impulse"].tobytes(), got[i]["normal_impulse"].tobytes()) == \
                   (bc["n_contacts"], bc["impulse"].tobytes(), bc["normal_impulse"].tobytes()), i
        if r["other"] == ANY:
            assert got[i]["n_contacts"] == bc["n_contacts"] and got[i]["normal_impulse"].tobytes() == bc["normal_impulse"].tobytes(), i
        if r["other"] == STATIC:
            assert got[i]["n_contacts"] == bc["n_terrain"], i
    hit = got["n_contacts"] > 0
    assert same_bytes(got[~hit], no_match(int(np.sum(~hit)))) and np.any(hit) and np.any(~hit)
    if tick == 30:
        assert len(s["lists"][1]) == 157 and len(s["lists"][2]) == 952
        assert np.any(got["record"][hit] != [TC.chain(s["lists"][int(r["world"])], int(r["body"]), int(r["other"]))[0][0] for r in rig[hit]])


# ---- 2: the hub ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hub_first", [True, False], ids=["hub_is_b_300_times", "hub_own_range_of_300"])
def test_hub_a_chain_longer_than_a_workgroup(ctx, hub_first):
    sc, hub = OC.hub_scene(hub_first)
    for t, b, lists in run_beside_oracle(ctx, [sc], (1, 2)):
        rig = TC.hub_sensors(lists[0], hub, 301)
        got, _, _ = check(b, rig, lists, f"hub tick {t}")
        assert len(lists[0]) == 300 and got["n_contacts"][0] == got["n_contacts"][1] == 300 and got[2:3].tobytes() == no_match(1).tobytes()
        pairs = got[3:-1].reshape(-1, 3)                       # (hub, x), (x, hub), (x, any) for the small spheres x
        assert np.all(pairs["n_contacts"] == 1) and np.all(pairs["partner"][:, 0] != hub) and np.all(pairs["partner"][:, 1:] == hub)
        assert np.all(pairs["record"][:, 0] == pairs["record"][:, 1])
        assert got[-1:].tobytes() == no_match(1).tobytes()
        assert b.counter("query_launches") == 1


# ---- 3: more sensors on one world than a work item holds -------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [257, 600])
def test_more_than_256_sensors_in_one_world(piles, count):
    b, s = piles["b"], piles["snaps"][30]
    k = TC.SMALL
    rig = TC.many_on_one_world(s["lists"][k], piles["lengths"][k], k, count)
    assert len(rig) == count and np.all(rig["world"] == k)
    b.set_touches(rig)
    got = b.read_touches()
    assert b.counter("query_launches") == 1
    same_records(got, TC.fold_rig(rig, s["lists"], s["qs"]), f"{count} sensors on the 96-sphere world")
    uniq, inverse = np.unique(rig, return_inverse=True)
    alone = np.zeros(len(uniq), mgf_amd.TOUCH_REPORT_DTYPE)
    for i in range(len(uniq)):
        b.set_touches(uniq[i:i + 1])
        alone[i] = b.read_touches()[0]
    same_records(got, alone[inverse.reshape(-1)], "every report against the one its sensor gets alone")
    assert np.sum(got["n_contacts"] >= 2) > 50 and np.sum(got["n_contacts"] == 0) > 50


# ---- 4: capsules over a heightfield -------------------------------------------------------------------------------------------------------
def test_capsules_over_a_heightfield(ctx):
    scs = OC.capsule_scenes()
    lengths = lengths_of(scs)
    for t, b, lists in run_beside_oracle(ctx, scs, (20, 40)):
        rig = TC.rig_of(lists, lengths)
        got, mine, qs = check(b, rig, lists, f"capsules tick {t}")
        static = rig["other"] == STATIC
        assert got["n_contacts"][static].max() >= 2                      # two contacts a face: two records of one body against the terrain
        framed = (rig["flags"] == FRAME) & (got["n_contacts"] > 0)
        world_frame = rig.copy()
        world_frame["flags"] = 0
        plain = TC.fold_rig(world_frame[framed], lists, qs)
        assert np.sum(framed) >= 2                                       # (tick 20: few capsules have landed)
        for f in ("impulse", "push", "arm"):
            assert np.any(np.ascontiguousarray(plain[f]).view(np.uint32) != np.ascontiguousarray(got[f][framed]).view(np.uint32)), f
    assert all(np.sum(lists[k]["b"] >= 0) > 0 for k in range(2))


# ---- 5: obstacles count as Static ---------------------------------------------------------------------------------------------------------
def test_obstacle_contacts_count_under_static(ctx):
    scs = BC.obstacle_scenes()
    lengths = lengths_of(scs)
    ows = [BC.oracle_with_obstacles(sc) for sc in scs]
    for t, b, lists in run_beside_oracle(ctx, scs, (20, 40), ows=ows, own_terrain=True):
        rig = TC.rig_of(lists, lengths)
        got, _, _ = check(b, rig, lists, f"obstacles tick {t}")
    bare = lists[BC.BARE]                                                 # no terrain: every record against Static is an obstacle's
    assert scs[BC.BARE]["terrain"] is None and np.sum(bare["b"] < 0) > 0
    on_ring = (rig["world"] == BC.BARE) & (rig["other"] == STATIC) & (got["n_contacts"] > 0)
    assert np.any(on_ring) and np.all(got["partner"][on_ring] == -1)


# ---- 6: bodies of several components ------------------------------------------------------------------------------------------------------
def test_bodies_of_several_components_are_not_refused_and_a_manifold_folds_in_list_order(ctx):
    scs = PC.six_scenes()
    lengths = lengths_of(scs)
    for t, b, lists in run_beside_oracle(ctx, scs, (TC.PARTS_TICK,), ows=PC.oracles(scs), own_terrain=True):
        with pytest.raises(mgf_amd.MgfError):
            b.read_zones(4)                                               # (the calls that read shapes are refused on this batch)
        rig = TC.rig_of(lists, lengths)
        got, _, _ = check(b, rig, lists, "parts")
        assert b.counter("query_launches") == 1
        for k in (PC.DUMBBELLS, PC.JACKS):
            assert PC.largest_manifold(lists[k]) >= 2
            pair = (rig["world"] == k) & (rig["other"] >= 0) & (got["n_contacts"] >= 2)
            assert np.any(pair), k
            for i in np.flatnonzero(pair):
                ch = TC.chain(lists[k], int(rig["body"][i]), int(rig["other"][i]))
                idx = [c for c, _, _ in ch]
                assert idx == list(range(idx[0], idx[0] + len(idx))) and got["record"][i] in idx       # consecutive records: a manifold
                ni = lists[k]["normal_impulse"][idx]
                assert got["record"][i] == idx[int(np.argmax(ni))] and got["strongest_impulse"][i] == ni.max()
        out = np.zeros((len(rig), 16), np.int32)
        import torch
        dev = torch.zeros((len(rig), 16), dtype=torch.int32, device="cuda")
        b.read_touches_dev(dev)
        torch.cuda.synchronize()
        out[:] = dev.cpu().numpy()
        assert out.tobytes() == got.tobytes()


# ---- 7: iters = 0 -------------------------------------------------------------------------------------------------------------------------
def test_no_solver_iterations_counts_without_impulses(ctx):
    scs = BQ.pile_scenes()[1:3]
    lengths = lengths_of(scs)
    for t, b, lists in run_beside_oracle(ctx, scs, (3,), iters=0):
        rig = TC.rig_of(lists, lengths)
        got, _, _ = check(b, rig, lists, "iters = 0")
        hit = got["n_contacts"] > 0
        assert got["n_contacts"].sum() > 100 and np.any(got["n_contacts"] >= 2)
        for f in ("impulse", "normal_impulse", "strongest_impulse"):
            assert not np.any(np.ascontiguousarray(got[f]).view(np.uint32)), f"{f} is not exactly +0"
        first = [TC.chain(lists[int(r["world"])], int(r["body"]), int(r["other"]))[0][0] for r in rig[hit]]
        assert got["record"][hit].tolist() == first                       # every ni is +0: nothing is ever stronger than the first match


# ---- 8: around the list's lifetime --------------------------------------------------------------------------------------------------------
def test_before_a_tick_behind_added_bodies_and_a_short_buffer(ctx, piles):
    scs, s = piles["scs"], piles["snaps"][30]
    rig = s["rig"]
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs)
    assert b.touch_count() == 0 and len(b.read_touches()) == 0 and b.counter("query_launches") == 0
    b.set_touches(rig)
    same_records(b.read_touches(), no_match(len(rig)), "before any tick")
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    b.step(dt, iters, 30)
    same_records(b.read_touches(), s["got"], "at tick 30, the rig set before the first tick")
    lib = mgf_amd.load_library()
    buf = np.full(len(rig) + 1, 0x5A, np.uint8).repeat(64).view(mgf_amd.TOUCH_REPORT_DTYPE)
    before = buf.tobytes()
    assert lib.mgf_batch_read_touches(b._h, buf.ctypes.data, len(rig) - 1) == _capi.ERR_CAPACITY and buf.tobytes() == before
    assert lib.mgf_batch_read_touches(b._h, None, len(rig)) == _capi.ERR_INVALID and "NULL" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_read_touches(b._h, buf.ctypes.data, -1) == _capi.ERR_INVALID and "negative" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_read_touches(b._h, buf.ctypes.data, len(rig)) == 0 and buf[:len(rig)].tobytes() == s["got"].tobytes() and buf[len(rig):].tobytes() == before[-64:]
    # what set refuses with a handle in hand: the rig stays as it was
    n1 = piles["lengths"][1]
    for world, body, other, flags, word in ((5, 0, ANY, 0, "world index"), (-1, 0, ANY, 0, "world index"), (1, n1, ANY, 0, "body index"), (1, -1, ANY, 0, "body index"),
                                            (3, 0, ANY, 0, "body index"), (1, 0, -4, 0, "other"), (1, 0, n1, 0, "other"), (1, 7, 7, 0, "its own body"),
                                            (1, 0, ANY, 2, "MGF_TOUCH_BODY_FRAME"), (1, 0, 3, -1, "MGF_TOUCH_BODY_FRAME")):
        bad = np.concatenate([rig[:3], np.array([(world, body, other, flags)], mgf_amd.TOUCH_DTYPE)])
        with pytest.raises(mgf_amd.MgfError, match=word):
            b.set_touches(bad)
        assert b.touch_count() == len(rig)
    same_records(b.read_touches(), s["got"], "behind the refused set calls")
    # write_state: the list does not move, the body frame follows the new q at once
    st = b.state(2)
    turn = np.float32([np.cos(0.35), 0.0, np.sin(0.35), 0.0])
    newq = np.tile(turn, (len(st["q"]), 1)).astype(np.float32)
    b.write_state(2, x=(st["x"] + np.float32([0.0, 5.0, 0.0])).astype(np.float32), q=newq)
    got = b.read_touches()
    world_frame = (rig["flags"] == 0) | (rig["world"] != 2) | (s["got"]["n_contacts"] == 0)
    same_records(got[world_frame], s["got"][world_frame], "world-frame reports after write_state")
    qs = dict(s["qs"])
    qs[2] = b.state(2)["q"]
    assert qs[2].tobytes() == newq.tobytes()
    same_records(got, TC.fold_rig(rig, s["lists"], qs), "body-frame reports follow the new q")
    assert np.sum(~world_frame) > 3 and all(got[i:i + 1].tobytes() != s["got"][i:i + 1].tobytes() for i in np.flatnonzero(~world_frame))
    # copy_worlds carries the list: the destination's sensors answer as the source's
    dst = mgf_amd.WorldBatch.from_scenes(ctx, scs)
    dst.set_touches(rig)
    dst.copy_worlds([1, 2, 4], b, [1, 2, 4])
    same_records(dst.read_touches(), got, "the destination of copy_worlds")
    # bodies added behind a tick: every list is empty until the next tick, and every sensor stays on the body it named
    extra = scenes.sphere_pile(1, 1, 1)
    new = extra["comps"].copy()
    new["p"] += np.float32([0.0, 30.0, 0.0])
    b.add_bodies(0, new, extra["mass"], extra["restitution"], extra["friction"], extra["force"])
    assert all(len(b.constraints(k)) == 0 for k in range(5)) and b.touch_count() == len(rig)
    same_records(b.read_touches(), no_match(len(rig)), "behind added bodies")
    b.step(dt, iters)
    lists = {k: b.constraints(k) for k in worlds_of(rig)}
    same_records(b.read_touches(), TC.fold_rig(rig, lists, {k: b.state(k)["q"] for k in lists}), "after the next tick")
    b.set_touches(rig[:0])
    assert b.touch_count() == 0 and len(b.read_touches()) == 0 and b.counter("query_launches") == 0


def test_a_tick_run_again_for_capacity(ctx):
    scs = BQ.pile_scenes()
    lengths = lengths_of(scs)
    for t, b, lists in run_beside_oracle(ctx, scs, (12,), options=dict(cons_per_body=1)):
        assert b.counter("capacity_retries") > 0 and len(lists[2]) > 512
        check(b, TC.rig_of(lists, lengths, skip=(TC.NO_SENSOR_WORLD,)), lists, "behind a capacity re-run")


# ---- 9: into device memory ----------------------------------------------------------------------------------------------------------------
def test_read_touches_dev(ctx, piles):
    import torch
    b, s = piles["b"], piles["snaps"][30]
    rig = s["rig"]
    n = len(rig)
    b.set_touches(rig)
    want = b.read_touches()
    for dtype in (torch.int32, torch.float32):
        dev = torch.full((n, 16), FILL, dtype=torch.int32, device="cuda").view(dtype)
        torch.cuda.synchronize()
        b.read_touches_dev(dev)
        assert b.counter("query_launches") == 1
        torch.cuda.synchronize()
        assert dev.view(torch.int32).cpu().numpy().tobytes() == want.tobytes()
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    dev = torch.full((n + 1, 16), FILL, dtype=torch.int32, device="cuda")
    host = np.zeros((n, 16), np.int32)
    short = torch.full((n - 1, 16), FILL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert lib.mgf_batch_read_touches_dev(b._h, host.ctypes.data, n) == INV and "out_dev" in err()              # host memory
    # a short allocation: torch hands small tensors out of blocks of 2 MiB, so only a rig whose reports exceed that is certainly too long
    many = 40000
    b.set_touches(np.repeat(rig[:1], many))
    assert 64 * many > (2 << 20) > short.numel() * 4
    assert lib.mgf_batch_read_touches_dev(b._h, short.data_ptr(), many) == INV and "allocation ends" in err()
    b.set_touches(rig)
    assert lib.mgf_batch_read_touches_dev(b._h, dev.data_ptr() + 2, n) == INV and "aligned" in err()            # misaligned
    assert lib.mgf_batch_read_touches_dev(b._h, dev.data_ptr(), n - 1) == _capi.ERR_CAPACITY
    assert lib.mgf_batch_read_touches_dev(b._h, None, n) == INV and "NULL" in err()
    assert lib.mgf_batch_read_touches_dev(b._h, dev.data_ptr(), -1) == INV and "negative" in err()
    torch.cuda.synchronize()
    assert bool(torch.all(dev == FILL)) and bool(torch.all(short == FILL)) and not host.any()                      # nothing was enqueued
    assert lib.mgf_batch_read_touches_dev(b._h, dev.data_ptr() + 4, n) == 0                                       # 4-byte alignment is enough
    torch.cuda.synchronize()
    flat = dev.reshape(-1).cpu().numpy()
    assert flat[1:1 + 16 * n].tobytes() == want.tobytes() and flat[0] == FILL and np.all(flat[1 + 16 * n:] == FILL)
    with pytest.raises(ValueError):
        b.read_touches_dev(torch.zeros((n, 16), dtype=torch.int32))
    with pytest.raises(ValueError):
        b.read_touches_dev(torch.zeros((n, 15), dtype=torch.int32, device="cuda"))


# ---- 10: the tick is untouched ------------------------------------------------------------------------------------------------------------
def test_the_tick_is_untouched(ctx):
    scs = [scenes.sphere_pile(4, 6, 4, seed=5), scenes.capsule_field(3, 2, 3)]
    scs[1] = dict(scs[1], terrain=scs[0]["terrain"])
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    a, b = mgf_amd.WorldBatch.from_scenes(ctx, scs), mgf_amd.WorldBatch.from_scenes(ctx, scs)
    rows = [(k, x, other, x & 1) for k in range(2) for x in range(0, len(scs[k]["comps"]), 3) for other in (ANY, STATIC, ANY_BODY, (x + 1) % len(scs[k]["comps"]))]
    b.set_touches(np.array(rows, mgf_amd.TOUCH_DTYPE))
    contacts = 0
    for _ in range(30):
        a.step(dt, iters)
        b.step(dt, iters)
        contacts += int(b.read_touches()["n_contacts"].sum())
    assert contacts > 0 and a.counter("launches_per_tick") == b.counter("launches_per_tick") == 6
    for k in range(2):
        sa, sb = a.state(k), b.state(k)
        for f in STATE:
            assert bits_equal(sa[f], sb[f]), (k, f)
        assert same_bytes(a.constraints(k), b.constraints(k)), f"world {k}: the constraint lists differ"


# ---- 11: independence ---------------------------------------------------------------------------------------------------------------------
def test_an_answer_depends_on_its_world_only(ctx, piles):
    scs, s = piles["scs"], piles["snaps"][30]
    rig = s["rig"]
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    rb = mgf_amd.WorldBatch.from_scenes(ctx, scs[::-1])
    rb.step(dt, iters, 30)
    rev = rig.copy()
    rev["world"] = 4 - rig["world"]
    rb.set_touches(rev)
    same_records(rb.read_touches(), s["got"], "a batch built in reverse order")
    rb.set_touches(rev[::-1].copy())
    same_records(rb.read_touches(), s["got"][::-1], "... and the rig in reverse order")
    one = mgf_amd.WorldBatch.from_scenes(ctx, [scs[2]])
    one.step(dt, iters, 30)
    of2 = rig[rig["world"] == 2].copy()
    of2["world"] = 0
    one.set_touches(of2)
    same_records(one.read_touches(), s["got"][rig["world"] == 2], "world 2 alone")


# ---- 12: the launch count -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_worlds", [1, 300])
def test_one_launch_whatever_the_worlds(ctx, piles, n_worlds):
    scs, s = piles["scs"], piles["snaps"][30]
    b = mgf_amd.WorldBatch.from_scenes(ctx, [scs[1]] * n_worlds)        # (300: more worlds than compute units)
    base = s["rig"][s["rig"]["world"] == 1]
    rig = np.concatenate([base] * n_worlds)
    rig["world"] = np.repeat(np.arange(n_worlds, dtype=np.int32), len(base))
    assert b.read_touches().shape == (0,) and b.counter("query_launches") == 0          # an empty rig
    b.set_touches(rig)
    b.step(float(scs[0]["dt"]), scs[0]["iters"], 30)
    got = b.read_touches()                                               # directly behind a step: no collider gather
    assert b.counter("query_launches") == mgf_amd.BATCH_TOUCH_LAUNCHES == 1
    same_records(got, np.tile(s["got"][s["rig"]["world"] == 1], n_worlds), f"{n_worlds} copies of the 96-sphere world")
