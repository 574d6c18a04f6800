"""The box zones of a batch (mgf_batch_set_zones / _read_zones / _read_zones_dev / _overlap_first_dev; WorldBatch.set_zones / .read_zones /
.read_zones_dev / .overlap_first_dev) against their definition on the SAME batch at the same moment: the boxes equal the numpy
restatement of c = x + rotate(q, p) over state() byte for byte (tests/batch_zone_cases.py), and every record equals the restated record
of what overlap_boxes reports for those boxes, with the zone's own body removed where it asks for that - for k = 0, 1, 8, 64 and 1024,
before a tick and after three, on bodies that have turned, for zones on a body, in the world, with NaN and with negative extents; the
device form equals the host form; overlap_first_dev equals the same restatement over the caller's boxes; nothing of the tick's state is
touched; a zone follows write_state at once and stays on the body it named when bodies are added; the three rigs leave one another
alone; the launch counts and the refusals are the header's.  No test hands a device call a host pointer or a short buffer: those
refusals are read in the source (tests/test_world_batch_zones_host.py)."""
import numpy as np
import pytest

from tests import batch_sensor_cases as SC
from tests import batch_zone_cases as ZC

pytestmark = pytest.mark.gpu
FILL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    import mgf_amd
    c = mgf_amd.Context(0)
    yield c
    c.close()


def _sync():
    import torch
    torch.cuda.synchronize()


def _lengths(b):
    return [b.world_len(k) for k in range(b.n_worlds)]


def _make(ctx, scs):
    import mgf_amd
    return mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)


def _step(b, scs, n=1):
    b.step(float(scs[0]["dt"]), scs[0]["iters"], n)


def _lists(b, rig):
    """(boxes, offsets, bodies): the restated boxes from state() and what overlap_boxes reports for them on this batch, now"""
    bx = ZC.boxes(rig, b.state(), _lengths(b))
    off, bodies = b.overlap_boxes(rig["world"], bx)
    return bx, off, bodies


def _read_dev(b, k, boxes=True):
    """read_zones_dev between two waits for the whole device; `out` and `boxes` start as 0x5A bytes: a word the call does not write shows"""
    import torch
    n = b.zone_count()
    out = torch.full((n, 1 + k), FILL, dtype=torch.int32, device="cuda")
    bt = torch.full((n, 6), FILL, dtype=torch.int32, device="cuda").view(torch.float32) if boxes else None
    _sync()
    b.read_zones_dev(out, boxes=bt)
    _sync()
    return out.cpu().numpy(), (bt.cpu().numpy() if boxes else None)


def _assert_reads(b, rig, note, ks=ZC.KS, repeats=1):
    """every form of a read against the definition, for every k; returns the counts"""
    bx, off, bodies = _lists(b, rig)
    ign = ZC.ignore_of(rig)
    for k in ks:
        want = ZC.records(off, bodies, ign, k)
        for rep in range(repeats):
            count, first, got_bx = b.read_zones(k, boxes=True)
            assert got_bx.tobytes() == bx.tobytes(), (note, k, rep, "boxes, host form", np.flatnonzero(np.any(got_bx.view(np.uint32) != bx.view(np.uint32), axis=1))[:8])
            got = np.concatenate([count[:, None], first], axis=1)
            assert got.tobytes() == want.tobytes(), (note, k, rep, "host form", np.flatnonzero(np.any(got != want, axis=1))[:8])
            count, first = b.read_zones(k)
            assert np.concatenate([count[:, None], first], axis=1).tobytes() == want.tobytes(), (note, k, rep, "host form without boxes")
            got, got_bx = _read_dev(b, k)
            assert got_bx.tobytes() == bx.tobytes(), (note, k, rep, "boxes, device form")
            assert got.tobytes() == want.tobytes(), (note, k, rep, "device form", np.flatnonzero(np.any(got != want, axis=1))[:8])
            got, _ = _read_dev(b, k, boxes=False)
            assert got.tobytes() == want.tobytes(), (note, k, rep, "device form without boxes")
    return (np.diff(off) - np.array([ign[i] in bodies[int(off[i]):int(off[i + 1])] for i in range(len(rig))])).astype(np.int64)


def _spin(b, rig, seed):
    """angular velocities for the bodies that carry a zone (their linear ones kept)"""
    on = rig[rig["body"] >= 0]
    key = np.unique(on["world"].astype(np.int64) * 4096 + on["body"])
    w, bd = (key // 4096).astype(np.int32), (key % 4096).astype(np.int32)
    om = np.random.default_rng(seed).uniform(-9.0, 9.0, (len(w), 3)).astype(np.float32)
    b.set_velocities(w, bd, b.get(w, bd)["linear"], om)
    return w, bd


def _turned(ctx, seed=5):
    scs = ZC.zone_scenes()
    rig, role = ZC.zone_rig(scs)
    b = _make(ctx, scs)
    w, bd = _spin(b, rig, seed)
    _step(b, scs, ZC.TICKS)
    q = b.state()["q"][SC.offsets(_lengths(b))[w] + bd]
    away = np.sum(q != np.float32([1, 0, 0, 0]), axis=1) >= 2
    assert 2 * int(np.sum(away)) >= len(w), (int(np.sum(away)), len(w))     # a rig on unrotated bodies tests nothing of rotate
    b.set_zones(rig)
    return b, rig, role, scs


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_records_and_boxes_equal_the_definition_byte_for_byte_before_a_tick_and_after_three(ctx):
    scs = ZC.zone_scenes()
    rig, role = ZC.zone_rig(scs)
    b = _make(ctx, scs)
    assert _lengths(b) == [5, 0, 1, 300] and b.zone_count() == 0
    # before any tick: the batch still in its host mirror, the colliders as the bodies were added
    b.set_zones(rig)
    assert b.zone_count() == len(rig) == sum(ZC.COUNTS)
    count = _assert_reads(b, rig, "before any tick")
    print("counts before any tick:", {int(c): int(n) for c, n in zip(*np.unique(count, return_counts=True))})
    for k in (1, 8, 64):   # the cases the scenes were built for (tests/test_world_batch_zones_host.py holds them to the oracle)
        assert np.any(count == 0) and np.any(count > k) and (k == 1 or np.any((count > 0) & (count < k)))
    assert np.any(count == 1) and count.max() == 300
    assert np.all(count[(role == ZC.NAN_P) | (role == ZC.NAN_R) | (role == ZC.FAR)] == 0) and np.all(count[rig["world"] == ZC.WE] == 0)
    w, bd = _spin(b, rig, seed=5)
    _step(b, scs, ZC.TICKS)
    q = b.state()["q"][SC.offsets(_lengths(b))[w] + bd]
    assert 2 * int(np.sum(np.sum(q != np.float32([1, 0, 0, 0]), axis=1) >= 2)) >= len(w)
    count = _assert_reads(b, rig, "after three ticks", repeats=2)
    print("counts after three ticks:", {int(c): int(n) for c, n in zip(*np.unique(count, return_counts=True))})
    assert np.any(count == 0) and np.any(count > 64) and np.any((count > 1) & (count < 8))
    # the rig given in reversed order: the same answers, zone by zone (the cover is then the FIRST of its world: one lane walks its list)
    before = b.read_zones(8, boxes=True)
    b.set_zones(rig[::-1].copy())
    _assert_reads(b, rig[::-1], "reversed", ks=(8, 1024))
    after = b.read_zones(8, boxes=True)
    assert all(x[::-1].tobytes() == y.tobytes() for x, y in zip(before, after))
    # through the arrays of set_zones too (what the ZONE_DTYPE form is built from)
    b.set_zones(rig["world"], rig["body"], rig["p"], rig["r"], (rig["flags"] & 1).astype(bool))
    _assert_reads(b, rig, "by arrays", ks=(8,))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", ZC.PERS)
def test_overlap_first_dev_equals_the_restatement_over_the_callers_boxes(ctx, per):
    import torch
    scs = ZC.zone_scenes()
    b = _make(ctx, scs)
    for moment in ("before any tick", "after three ticks"):
        bx, ign = ZC.fixed_boxes(scs, per)
        world = np.repeat(np.arange(len(scs), dtype=np.int32), per)
        off, bodies = b.overlap_boxes(world, bx)
        removed = np.array([ign[i] in bodies[int(off[i]):int(off[i + 1])] for i in range(len(bx))])
        assert np.any(removed) and np.any((ign >= np.repeat(_lengths(b), per)) | (ign < -1))      # an ignore that takes a body out; one that names none
        d_bx, d_ign = torch.from_numpy(bx).cuda(), torch.from_numpy(ign).cuda()
        for k in ZC.KS:
            for with_ignore in (True, False):
                want = ZC.records(off, bodies, ign if with_ignore else np.full(len(bx), -1), k)
                out = torch.full((len(bx), 1 + k), FILL, dtype=torch.int32, device="cuda")
                _sync()
                b.overlap_first_dev(d_bx, out, ignore=d_ign if with_ignore else None)
                _sync()
                got = out.cpu().numpy()
                assert got.tobytes() == want.tobytes(), (moment, per, k, with_ignore, np.flatnonzero(np.any(got != want, axis=1))[:8])
                assert b.counter("query_launches") == 1             # (overlap_boxes has gathered the colliders behind the step)
        if moment == "before any tick":
            _step(b, scs, ZC.TICKS)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def _everything(b):
    st = b.state()
    return [st[k].tobytes() for k in ("x", "q", "v", "omega", "delta")] + [b.constraints(k).tobytes() for k in range(b.n_worlds)]


def test_a_step_after_a_read_is_bit_identical_to_the_twins_step_without_one(ctx):
    import torch
    scs = ZC.zone_scenes()
    rig, _ = ZC.zone_rig(scs)
    a, b = _make(ctx, scs), _make(ctx, scs)
    for t in (a, b):
        _spin(t, rig, seed=6)
        _step(t, scs, ZC.TICKS)
    assert _everything(a) == _everything(b)
    b.set_zones(rig)
    bx, ign = ZC.fixed_boxes(scs, 3)
    out = torch.zeros((len(bx), 9), dtype=torch.int32, device="cuda")
    for k in (8, 1024):
        b.read_zones(k, boxes=True)
        _read_dev(b, k)
    b.overlap_first_dev(torch.from_numpy(bx).cuda(), out, ignore=torch.from_numpy(ign).cuda())
    _sync()
    assert _everything(a) == _everything(b)          # (a read writes nothing a reader of the state sees)
    _step(a, scs)
    _step(b, scs)
    _read_dev(b, 8)
    assert _everything(a) == _everything(b)
    _step(a, scs, 2)
    _step(b, scs, 2)
    assert _everything(a) == _everything(b)


# ---- 4, 5, 6: these change the batch, so each has one of its own ----------------------------------------------------------------------------
def test_a_zone_follows_write_state_at_once(ctx):
    b, rig, role, scs = _turned(ctx)
    k = ZC.W300
    st = b.state(k)
    rng = np.random.default_rng(8)
    q = rng.normal(0, 1, st["q"].shape)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    x = (st["x"] + rng.uniform(-0.6, 0.6, st["x"].shape)).astype(np.float32)
    before = b.read_zones(8, boxes=True)
    cols = b.colliders(k).tobytes()
    b.write_state(k, x=x, q=q)
    assert np.array_equal(b.state(k)["q"], q) and b.colliders(k).tobytes() == cols      # the colliders a query sees have not moved
    _assert_reads(b, rig, "behind write_state", ks=(8, 1024))
    after = b.read_zones(8, boxes=True)
    moved = np.any(after[2] != before[2], axis=1)
    on = (rig["world"] == k) & (rig["body"] >= 0) & ~np.isnan(rig["p"]).any(axis=1)
    assert np.all(moved[on]) and not np.any(moved[~on & ~np.isnan(before[2]).any(axis=1)])    # every zone on a body of that world, and no other
    assert after[0].tobytes() != before[0].tobytes()
    _step(b, scs)                                 # and behind the next tick, which moves the colliders
    _assert_reads(b, rig, "a tick behind write_state", ks=(8,))


def test_bodies_added_to_a_middle_world_leave_every_zone_on_its_body(ctx):
    b, rig, role, scs = _turned(ctx)
    old = SC.offsets(_lengths(b))
    mid = scs[ZC.W1]
    comps = mid["comps"][:1].repeat(2)
    comps["p"] += np.float32([[0.0, 1.5, 0.0], [0.0, 3.0, 0.0]])
    b.add_bodies(ZC.W1, comps, 1.0, float(mid["restitution"][0]), float(mid["friction"][0]), mid["force"][:1].repeat(2, axis=0))
    assert _lengths(b) == [5, 0, 3, 300] and b.zone_count() == len(rig)
    assert np.any(SC.offsets(_lengths(b))[rig["world"]] != old[rig["world"]])      # flat indices have moved under the rig
    count = _assert_reads(b, rig, "behind add_bodies", ks=(8, 1024))                # the reference names the same (world, body)
    _step(b, scs)
    count = _assert_reads(b, rig, "a tick behind add_bodies", ks=(8,), repeats=2)
    assert np.any(count > 8)
    # a body the world did not hold before can carry a zone now
    more = np.concatenate([rig, np.array([(ZC.W1, 2, (0, 0, 0), (0.1, 0.1, 0.1), 0, 0)], rig.dtype)])
    b.set_zones(more)
    count = _assert_reads(b, more, "a zone on an added body", ks=(1,))
    assert count[-1] >= 1


def test_zones_sensors_and_cameras_do_not_disturb_one_another(ctx):
    from mgf_amd import _capi
    b, rig, role, scs = _turned(ctx)
    b.set_zones(np.zeros(0, _capi.ZONE_DTYPE))
    rng = np.random.default_rng(12)
    sw = np.full(40, ZC.W300, np.int32)
    b.set_sensors(sw, rng.integers(0, 300, 40).astype(np.int32), (0.0, 0.0, 0.0), rng.normal(0, 1, (40, 3)).astype(np.float32), np.inf, True)
    b.set_cameras([dict(world=ZC.W5, body=0, p=(0.0, 6.0, 0.0), r=(np.sqrt(0.5), np.sqrt(0.5), 0.0, 0.0), tan_x=0.8, tan_y=0.8, width=12, height=9, far=30.0)])
    hits = b.cast_sensors(7)
    depth = b.cast_cameras(7)[0]
    assert np.any(hits["kind"] >= 0) and np.any(depth < 30.0)
    b.set_zones(rig)
    assert (b.zone_count(), b.sensor_count(), b.camera_count()) == (len(rig), 40, 1)
    _assert_reads(b, rig, "beside sensors and cameras", ks=(8,))
    assert b.cast_sensors(7).tobytes() == hits.tobytes() and b.cast_cameras(7)[0].tobytes() == depth.tobytes()
    zones = [a.tobytes() for a in b.read_zones(8, boxes=True)]
    b.set_sensors(sw[:0], sw[:0], np.zeros((0, 3)), np.zeros((0, 3)))
    b.set_cameras([])
    assert (b.zone_count(), b.sensor_count(), b.camera_count()) == (len(rig), 0, 0)
    assert [a.tobytes() for a in b.read_zones(8, boxes=True)] == zones
    b.set_sensors(sw, rng.integers(0, 300, 40).astype(np.int32), (0.0, 0.0, 0.0), (0.0, -1.0, 0.0), np.inf, True)
    other = b.cast_sensors(7)
    b.set_zones(rig[:3].copy())
    assert b.zone_count() == 3 and b.cast_sensors(7).tobytes() == other.tobytes()
    _assert_reads(b, rig[:3], "three zones left", ks=(8,))


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_counters_refusals_and_the_empty_rig(ctx):
    import torch
    import mgf_amd
    from mgf_amd import _capi
    scs = ZC.zone_scenes()
    rig, role = ZC.zone_rig(scs)
    b = _make(ctx, scs)
    K, ONE = 4, _capi.BATCH_ZONE_LAUNCHES
    assert b.n_worlds == K and ONE == 1
    launches = {}
    for name, r in (("one", rig[:1]), ("all", rig), ("600", np.resize(rig, 600))):
        b.set_zones(r.copy())
        assert b.zone_count() == len(r)
        skipped = b.counter("device_skipped")
        got = []
        for k in (0, 8, 1024):
            b.read_zones(k)
            got.append((b.counter("query_launches"), b.counter("query_run_ns")))
            _read_dev(b, k)
            got.append((b.counter("query_launches"), b.counter("query_run_ns")))
        launches[name] = got
        assert b.counter("device_skipped") == skipped
    assert launches["one"] == launches["all"] == launches["600"] == [(ONE, 0)] * 6, launches
    _step(b, scs)
    _read_dev(b, 8)
    assert b.counter("query_launches") == ONE + 1      # the collider gather behind a step, once
    _read_dev(b, 8)
    assert b.counter("query_launches") == ONE
    _step(b, scs)
    b.read_zones(8)
    assert b.counter("query_launches") == ONE + 1
    b.read_zones(8)
    assert b.counter("query_launches") == ONE
    # refused on the host, the rig as it was
    big = np.resize(rig, 600)
    at = int(np.flatnonzero(big["body"] >= 0)[5])
    n = b.zone_count()
    kept = [a.tobytes() for a in b.read_zones(8, boxes=True)]
    lens = _lengths(b)
    for field, value in (("world", -1), ("world", K), ("body", -2), ("body", lens[int(big["world"][at])]), ("flags", 2), ("flags", 3), ("flags", -1),
                         ("reserved", 1), ("reserved", -1)):
        bad = big.copy()
        bad[field][at] = value
        with pytest.raises(mgf_amd.MgfError) as e:
            b.set_zones(bad)
        assert e.value.status == _capi.ERR_INVALID and b.zone_count() == n, (field, value)
    bad = big.copy()
    bad["body"][at], bad["flags"][at] = -1, _capi.SENSOR_IGNORE_SELF           # fixed in the world: no body of its own to ignore
    with pytest.raises(mgf_amd.MgfError) as e:
        b.set_zones(bad)
    assert e.value.status == _capi.ERR_INVALID and "ignore" in str(e.value) and b.zone_count() == n
    bad = big.copy()
    bad["world"][at], bad["body"][at], bad["flags"][at] = ZC.WE, 0, 0           # the world without bodies holds no body 0
    with pytest.raises(mgf_amd.MgfError):
        b.set_zones(bad)
    lib = mgf_amd.load_library()
    out = np.zeros((n, 9), np.int32)
    dev = torch.zeros((n, 9), dtype=torch.int32, device="cuda")
    _sync()
    assert lib.mgf_batch_read_zones(b._h, 8, out.ctypes.data, None, n - 1) == _capi.ERR_CAPACITY
    assert lib.mgf_batch_read_zones_dev(b._h, 8, dev.data_ptr(), None, n - 1) == _capi.ERR_CAPACITY
    assert lib.mgf_batch_read_zones(b._h, 8, None, None, n) == _capi.ERR_INVALID          # (a rig that is not empty needs somewhere to go)
    assert lib.mgf_batch_read_zones_dev(b._h, 8, None, None, n) == _capi.ERR_INVALID
    for k in (-1, _capi.BATCH_MAX_BODIES + 1):
        assert lib.mgf_batch_read_zones(b._h, k, out.ctypes.data, None, n) == _capi.ERR_INVALID
        assert lib.mgf_batch_read_zones_dev(b._h, k, dev.data_ptr(), None, n) == _capi.ERR_INVALID
        assert lib.mgf_batch_overlap_first_dev(b._h, dev.data_ptr(), K, None, k, dev.data_ptr()) == _capi.ERR_INVALID
    boxes = torch.zeros((K * 2 + 1, 6), dtype=torch.float32, device="cuda")
    _sync()
    assert lib.mgf_batch_overlap_first_dev(b._h, boxes.data_ptr(), K * 2 + 1, None, 8, dev.data_ptr()) == _capi.ERR_INVALID     # no multiple of n_worlds
    assert "multiple" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_overlap_first_dev(b._h, boxes.data_ptr(), K, None, 8, boxes.data_ptr()) == _capi.ERR_INVALID           # out_dev is an input
    assert "overlaps" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_read_zones_dev(b._h, 8, dev.data_ptr(), dev.data_ptr(), n) == _capi.ERR_INVALID                          # the two outputs overlap
    assert "overlaps" in lib.mgf_last_error().decode()
    assert b.zone_count() == n and [a.tobytes() for a in b.read_zones(8, boxes=True)] == kept
    # no boxes: nothing enqueued
    b.overlap_first_dev(boxes[:0], dev[:0])
    assert b.counter("query_launches") == 0
    # n = 0 empties the rig; a read then enqueues nothing
    b.set_zones(np.zeros(0, _capi.ZONE_DTYPE))
    assert b.zone_count() == 0
    count, first = b.read_zones(8)
    assert count.shape == (0,) and first.shape == (0, 8) and b.counter("query_launches") == 0
    assert [a.shape for a in b.read_zones(0, boxes=True)] == [(0,), (0, 0), (0, 6)]
    b.read_zones_dev(torch.zeros((0, 9), dtype=torch.int32, device="cuda"), boxes=torch.zeros((0, 6), dtype=torch.float32, device="cuda"))
    assert b.counter("query_launches") == 0
