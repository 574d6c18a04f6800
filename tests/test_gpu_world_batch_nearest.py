"""The zones of a batch read nearest first (mgf_batch_read_zones_nearest / _read_zones_nearest_dev / _overlap_nearest_dev;
WorldBatch.read_zones_nearest / .read_zones_nearest_dev / .overlap_nearest_dev) against their definition on the SAME batch at the same
moment: the list of a zone is what overlap_boxes reports for its restated box, the centres are those of colliders(), and the record -
the count, the bodies in ascending (d2, body index), -1 and +inf behind them - is tests/batch_nearest_cases.py's numpy restatement,
byte for byte: for k = 0, 1, 8 and 32, with and without the distances and the boxes, before a tick and after three on bodies that have
turned, with the rig reversed; on the tie world, where whole shells of bodies are equally far and the index alone decides; over the
caller's own boxes; nothing of the tick's state is touched; a zone follows write_state at once; the launch counts and the refusals are
the header's.  Outputs start as 0x5A bytes: a word a call does not write shows."""
import numpy as np
import pytest

from tests import batch_nearest_cases as NC
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


def _filled(shape, dtype):
    import torch
    t = torch.full(shape, FILL, dtype=torch.int32, device="cuda")
    return t if dtype == "int32" else t.view(torch.float32)


def _read_dev(b, k, dist2=True, boxes=True):
    n = b.zone_count()
    out = _filled((n, 1 + k), "int32")
    dt = _filled((n, k), "float32") if dist2 else None
    bt = _filled((n, 6), "float32") if boxes else None
    _sync()
    b.read_zones_nearest_dev(out, dist2=dt, boxes=bt)
    _sync()
    return out.cpu().numpy(), (dt.cpu().numpy() if dist2 else None), (bt.cpu().numpy() if boxes else None)


def _defined(b, rig):
    """what the definition needs of this batch, now: the restated boxes, overlap_boxes' lists for them, the colliders' tight centres"""
    lengths = _lengths(b)
    bx = ZC.boxes(rig, b.state(), lengths)
    off, bodies = b.overlap_boxes(rig["world"], bx)
    return bx, off, bodies, NC.tight_centres(b.colliders()), lengths


def _where(got, want):
    return np.flatnonzero(np.any(got.view(np.uint32).reshape(len(got), -1) != want.view(np.uint32).reshape(len(want), -1), axis=1))[:8]


def _assert_reads(b, rig, note, ks=NC.KS):
    """every form of a read against the definition, for every k; returns (the counts, the k = 32 records and distances)"""
    bx, off, bodies, centres, lengths = _defined(b, rig)
    ign = ZC.ignore_of(rig)
    last = None
    for k in ks:
        want, want_d = NC.records(off, bodies, ign, rig["world"], bx, centres, lengths, k)
        assert np.array_equal(want[:, 0], ZC.records(off, bodies, ign, 0)[:, 0])
        for dist2 in (True, False):
            for boxes in (True, False):
                got = b.read_zones_nearest(k, dist2=dist2, boxes=boxes)
                assert len(got) == 2 + dist2 + boxes
                rec = np.concatenate([got[0][:, None], got[1]], axis=1)
                assert rec.tobytes() == want.tobytes(), (note, k, dist2, boxes, "host form", _where(rec, want))
                if dist2:
                    assert got[2].tobytes() == want_d.tobytes(), (note, k, boxes, "distances, host form", _where(got[2], want_d))
                if boxes:
                    assert got[-1].tobytes() == bx.tobytes(), (note, k, dist2, "boxes, host form")
                rec, dd, gb = _read_dev(b, k, dist2, boxes)
                assert rec.tobytes() == want.tobytes(), (note, k, dist2, boxes, "device form", _where(rec, want))
                if dist2:
                    assert dd.tobytes() == want_d.tobytes(), (note, k, boxes, "distances, device form", _where(dd, want_d))
                if boxes:
                    assert gb.tobytes() == bx.tobytes(), (note, k, dist2, "boxes, device form")
        # word 0 is read_zones' count; where k holds the whole list the listed set is the first-k list's
        count, first = b.read_zones(k)
        assert np.array_equal(count, want[:, 0]), (note, k)
        whole = count <= k
        assert np.array_equal(np.sort(want[whole, 1:], axis=1), np.sort(first[whole], axis=1)), (note, k)
        last = (want, want_d)
    return want[:, 0].astype(np.int64), last


def _spin(b, rig, seed):
    """angular velocities for the bodies that carry a zone (their linear ones kept)"""
    on = rig[rig["body"] >= 0]
    key = np.unique(on["world"].astype(np.int64) * 4096 + on["body"])
    w, bd = (key // 4096).astype(np.int32), (key % 4096).astype(np.int32)
    om = np.random.default_rng(seed).uniform(-9.0, 9.0, (len(w), 3)).astype(np.float32)
    b.set_velocities(w, bd, b.get(w, bd)["linear"], om)
    return w, bd


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_records_distances_and_boxes_equal_the_definition_byte_for_byte_before_a_tick_and_after_three(ctx):
    scs, rig, role, tie = NC.scenes_and_rig()
    b = _make(ctx, scs)
    assert _lengths(b) == [5, 0, 1, 300, 27]
    b.set_zones(rig)
    count, (rec, dd) = _assert_reads(b, rig, "before any tick")
    print("counts before any tick:", {int(c): int(n) for c, n in zip(*np.unique(count, return_counts=True))})
    assert np.any(count == 0) and np.any(count == 1) and count.max() == 300 and np.sum(count > 32) >= 3 and np.any((count > 8) & (count < 32))
    assert np.any(dd.view(np.uint32) == 0)                                               # a d2 of exactly +0
    assert np.any((count > 8) & np.any(np.diff(rec[:, 1:9], axis=1) < 0, axis=1))     # nearest first is not index order
    assert np.all(count[(role == ZC.NAN_P) | (role == ZC.NAN_R) | (role == ZC.FAR)] == 0) and np.all(count[rig["world"] == ZC.WE] == 0)
    w, bd = _spin(b, rig, seed=5)
    _step(b, scs, ZC.TICKS)
    q = b.state()["q"][np.concatenate([[0], np.cumsum(_lengths(b))])[w] + bd]
    assert 2 * int(np.sum(np.sum(q != np.float32([1, 0, 0, 0]), axis=1) >= 2)) >= len(w)
    count, _ = _assert_reads(b, rig, "after three ticks")
    print("counts after three ticks:", {int(c): int(n) for c, n in zip(*np.unique(count, return_counts=True))})
    assert np.any(count == 0) and np.any(count > 32) and np.any((count > 1) & (count < 8))
    # the rig given in reversed order: the same answers, zone by zone (other work items, other lane splits)
    before = b.read_zones_nearest(8, dist2=True, boxes=True)
    b.set_zones(rig[::-1].copy())
    _assert_reads(b, rig[::-1], "reversed", ks=(8, 32))
    after = b.read_zones_nearest(8, dist2=True, boxes=True)
    assert all(x[::-1].tobytes() == y.tobytes() for x, y in zip(before, after))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_on_the_tie_world_the_index_alone_decides(ctx):
    scs, rig, role, (w_tie, nodes, centre, at) = NC.scenes_and_rig()
    b = _make(ctx, scs)
    b.set_zones(rig[at].copy())                        # fixed at the centre node; on the centre body; on it and ignoring it
    _assert_reads(b, rig[at], "the tie world")
    count, near, dd = b.read_zones_nearest(32, dist2=True)
    assert count.tolist() == [27, 27, 26]
    shells = sum(([v] * m for v, m in zip(NC.TIE_D2, NC.TIE_SHELLS)), [])
    for z in (0, 1):
        assert near[z, 0] == centre and dd[z, :27].tolist() == shells and np.all(near[z, 27:] == -1)
        assert dd[z, 27:].view(np.uint32).tolist() == [NC.INF_BITS] * 5
        for lo, hi in ((1, 7), (7, 19), (19, 27)):
            assert np.all(np.diff(near[z, lo:hi]) > 0), (z, lo, hi)
    assert near[0].tobytes() == near[1].tobytes() and dd[0].tobytes() == dd[1].tobytes()
    assert near[2, :26].tolist() == near[0, 1:27].tolist() and dd[2, :26].tolist() == shells[1:] and np.all(near[2, 26:] == -1)
    assert centre not in near[2].tolist()
    got = b.read_zones_nearest(8, dist2=True)                         # k = 8 cuts the shell of 12: the tie at the cut goes to the lower index
    assert got[1][0].tolist() == near[0, :8].tolist() and got[2][0].tolist() == shells[:8] and shells[7] == shells[8]


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", ZC.PERS)
def test_overlap_nearest_dev_equals_the_definition_over_the_callers_boxes(ctx, per):
    import torch
    scs = NC.scenes_and_rig()[0]
    b = _make(ctx, scs)
    for moment in ("before any tick", "after three ticks"):
        bx, ign = ZC.fixed_boxes(scs, per)
        world = np.repeat(np.arange(len(scs), dtype=np.int32), per)
        off, bodies = b.overlap_boxes(world, bx)
        centres, lengths = NC.tight_centres(b.colliders()), _lengths(b)
        removed = np.array([ign[i] in bodies[int(off[i]):int(off[i + 1])] for i in range(len(bx))])
        assert np.any(removed) and np.any((ign >= np.repeat(lengths, per)) | (ign < -1))      # an ignore that takes a body out; one that names none
        d_bx, d_ign = torch.from_numpy(bx).cuda(), torch.from_numpy(ign).cuda()
        for k in NC.KS:
            for with_ignore in (True, False):
                want, want_d = NC.records(off, bodies, ign if with_ignore else np.full(len(bx), -1), world, bx, centres, lengths, k)
                for dist2 in (True, False):
                    out = _filled((len(bx), 1 + k), "int32")
                    dt = _filled((len(bx), k), "float32") if dist2 else None
                    _sync()
                    b.overlap_nearest_dev(d_bx, out, dist2=dt, ignore=d_ign if with_ignore else None)
                    _sync()
                    got = out.cpu().numpy()
                    assert got.tobytes() == want.tobytes(), (moment, per, k, with_ignore, dist2, _where(got, want))
                    if dist2:
                        got = dt.cpu().numpy()
                        assert got.tobytes() == want_d.tobytes(), (moment, per, k, with_ignore, _where(got, want_d))
                    assert b.counter("query_launches") == 1             # (overlap_boxes has gathered the colliders behind the step)
        if moment == "before any tick":
            _step(b, scs, ZC.TICKS)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def _everything(b):
    st = b.state()
    return [st[k].tobytes() for k in ("x", "q", "v", "omega", "delta")] + [b.constraints(k).tobytes() for k in range(b.n_worlds)]


def test_a_step_after_the_reads_is_bit_identical_and_a_zone_follows_write_state_at_once(ctx):
    import torch
    scs, rig, role, tie = NC.scenes_and_rig()
    a, b = _make(ctx, scs), _make(ctx, scs)
    for t in (a, b):
        _spin(t, rig, seed=6)
        _step(t, scs, ZC.TICKS)
    assert _everything(a) == _everything(b)
    b.set_zones(rig)
    bx, ign = ZC.fixed_boxes(scs, 3)
    out, dd = torch.zeros((len(bx), 9), dtype=torch.int32, device="cuda"), torch.zeros((len(bx), 8), dtype=torch.float32, device="cuda")
    for k in (8, 32):
        b.read_zones_nearest(k, dist2=True, boxes=True)
        _read_dev(b, k)
    b.overlap_nearest_dev(torch.from_numpy(bx).cuda(), out, dist2=dd, ignore=torch.from_numpy(ign).cuda())
    _sync()
    assert _everything(a) == _everything(b)          # (a read writes nothing a reader of the state sees)
    _step(a, scs)
    _step(b, scs)
    _read_dev(b, 8)
    assert _everything(a) == _everything(b)
    _step(a, scs, 2)
    _step(b, scs, 2)
    assert _everything(a) == _everything(b)
    # a zone follows write_state at once; the colliders - the centres the distances are taken from - move at the next tick
    k = ZC.W300
    st = b.state(k)
    rng = np.random.default_rng(8)
    q = rng.normal(0, 1, st["q"].shape)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    x = (st["x"] + rng.uniform(-0.6, 0.6, st["x"].shape)).astype(np.float32)
    before = b.read_zones_nearest(8, dist2=True, boxes=True)
    cols = b.colliders(k).tobytes()
    b.write_state(k, x=x, q=q)
    assert b.colliders(k).tobytes() == cols
    _assert_reads(b, rig, "behind write_state", ks=(8,))
    after = b.read_zones_nearest(8, dist2=True, boxes=True)
    moved = np.any(after[3] != before[3], axis=1)
    on = (rig["world"] == k) & (rig["body"] >= 0) & ~np.isnan(rig["p"]).any(axis=1)
    assert np.all(moved[on]) and not np.any(moved[~on & ~np.isnan(before[3]).any(axis=1)])
    assert after[2].tobytes() != before[2].tobytes()
    _step(b, scs)
    _assert_reads(b, rig, "a tick behind write_state", ks=(8,))


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_counters_refusals_and_the_empty_rig(ctx):
    import torch
    import mgf_amd
    from mgf_amd import _capi
    scs, rig, role, tie = NC.scenes_and_rig()
    b = _make(ctx, scs)
    K, ONE = len(scs), _capi.BATCH_NEAREST_LAUNCHES
    assert b.n_worlds == K == 5 and ONE == 1
    b.set_zones(rig)
    n = b.zone_count()
    for k in (0, 8, 32):
        b.read_zones_nearest(k, dist2=True)
        assert (b.counter("query_launches"), b.counter("query_run_ns")) == (ONE, 0)
        _read_dev(b, k)
        assert (b.counter("query_launches"), b.counter("query_run_ns")) == (ONE, 0)
    _step(b, scs)
    _read_dev(b, 8)
    assert b.counter("query_launches") == ONE + 1      # the collider gather behind a step, once
    _read_dev(b, 8)
    assert b.counter("query_launches") == ONE
    _step(b, scs)
    b.read_zones_nearest(8)
    assert b.counter("query_launches") == ONE + 1
    b.read_zones_nearest(8)
    assert b.counter("query_launches") == ONE
    # refused, the rig and every output word as they were
    kept = [a.tobytes() for a in b.read_zones_nearest(8, dist2=True, boxes=True)]
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    out, hd = np.full((n, 9), FILL, np.int32), np.full((n, 8), FILL, np.int32)
    dev, dd, db = _filled((n, 34), "int32"), _filled((n, 33), "float32"), _filled((n, 6), "float32")
    boxes = torch.zeros((K * 2 + 1, 6), dtype=torch.float32, device="cuda")
    _sync()
    assert lib.mgf_batch_read_zones_nearest(b._h, 8, out.ctypes.data, hd.ctypes.data, None, n - 1) == _capi.ERR_CAPACITY
    assert lib.mgf_batch_read_zones_nearest_dev(b._h, 8, dev.data_ptr(), dd.data_ptr(), None, n - 1) == _capi.ERR_CAPACITY
    assert lib.mgf_batch_read_zones_nearest(b._h, 8, None, None, None, n) == INV          # (a rig that is not empty needs somewhere to go)
    assert lib.mgf_batch_read_zones_nearest_dev(b._h, 8, None, None, None, n) == INV
    for k in (-1, 33, _capi.BATCH_MAX_BODIES):
        assert lib.mgf_batch_read_zones_nearest(b._h, k, out.ctypes.data, hd.ctypes.data, None, n) == INV and "k is outside" in err(), k
        assert lib.mgf_batch_read_zones_nearest_dev(b._h, k, dev.data_ptr(), dd.data_ptr(), db.data_ptr(), n) == INV and "k is outside" in err(), k
        assert lib.mgf_batch_overlap_nearest_dev(b._h, boxes.data_ptr(), K, None, k, dev.data_ptr(), dd.data_ptr()) == INV and "k is outside" in err(), k
    assert lib.mgf_batch_overlap_nearest_dev(b._h, boxes.data_ptr(), K * 2 + 1, None, 8, dev.data_ptr(), None) == INV and "multiple" in err()
    assert lib.mgf_batch_overlap_nearest_dev(b._h, boxes.data_ptr(), K, None, 8, boxes.data_ptr(), None) == INV and "overlaps" in err()       # out_dev is an input
    assert lib.mgf_batch_overlap_nearest_dev(b._h, boxes.data_ptr(), K, None, 8, dev.data_ptr(), boxes.data_ptr()) == INV and "overlaps" in err()
    assert lib.mgf_batch_overlap_nearest_dev(b._h, boxes.data_ptr(), K, None, 8, dev.data_ptr(), dev.data_ptr()) == INV and "overlaps" in err()
    assert lib.mgf_batch_read_zones_nearest_dev(b._h, 8, dev.data_ptr(), dev.data_ptr(), None, n) == INV and "overlaps" in err()               # two outputs overlap
    assert lib.mgf_batch_read_zones_nearest_dev(b._h, 8, dev.data_ptr(), dd.data_ptr(), dd.data_ptr(), n) == INV and "overlaps" in err()
    assert lib.mgf_batch_read_zones_nearest_dev(b._h, 8, dev.data_ptr(), None, dev.data_ptr(), n) == INV and "overlaps" in err()
    _sync()
    for t in (dev, dd.view(torch.int32), db.view(torch.int32)):
        assert bool(torch.all(t == FILL))
    assert np.all(out == FILL) and np.all(hd == FILL) and not np.any(boxes.cpu().numpy())
    assert b.zone_count() == n and [a.tobytes() for a in b.read_zones_nearest(8, dist2=True, boxes=True)] == kept
    # a batch that holds a body of several components: refused as every call that reads shapes, nothing written
    from tests import batch_parts_cases as PC
    six = PC.six_scenes()
    parts = _make(ctx, [six[PC.JACKS], six[PC.PILE]])
    parts.set_zones([0, 1], [0, 0], r=(1.0, 1.0, 1.0))
    o2, d2, b2 = _filled((2, 3), "int32"), _filled((2, 2), "float32"), torch.ones((2, 6), dtype=torch.float32, device="cuda")
    for name, call in (("host", lambda: parts.read_zones_nearest(2, dist2=True)), ("dev", lambda: parts.read_zones_nearest_dev(o2, dist2=d2)),
                       ("boxes", lambda: parts.overlap_nearest_dev(b2, o2, dist2=d2))):
        with pytest.raises(mgf_amd.MgfError) as e:
            call()
        assert e.value.status == INV and "several components" in str(e.value), name
    _sync()
    assert bool(torch.all(o2 == FILL)) and bool(torch.all(d2.view(torch.int32) == FILL))
    # no boxes: nothing enqueued
    b.overlap_nearest_dev(boxes[:0], dev[:0, :9], dist2=dd[:0, :8])
    assert b.counter("query_launches") == 0
    # an empty rig: OK, nothing enqueued
    b.set_zones(np.zeros(0, _capi.ZONE_DTYPE))
    assert b.zone_count() == 0
    got = b.read_zones_nearest(8, dist2=True, boxes=True)
    assert [a.shape for a in got] == [(0,), (0, 8), (0, 8), (0, 6)] and b.counter("query_launches") == 0
    b.read_zones_nearest_dev(torch.zeros((0, 9), dtype=torch.int32, device="cuda"), dist2=torch.zeros((0, 8), dtype=torch.float32, device="cuda"),
                             boxes=torch.zeros((0, 6), dtype=torch.float32, device="cuda"))
    assert b.counter("query_launches") == 0
