"""The body-mounted ray sensors of a batch (mgf_batch_set_sensors / _cast_sensors / _cast_sensors_dev; WorldBatch.set_sensors /
.cast_sensors / .cast_sensors_dev) against their definition on the SAME batch at the same moment: the particles equal the numpy
restatement of P = x + rotate(q, p), D = rotate(q, d) over state() byte for byte (tests/batch_sensor_cases.py, held to the oracle by
tests/test_world_batch_sensors_host.py), and the hits equal raycast of those particles byte for byte - on bodies that have turned,
under every mask, before a tick and after three, call after call, whatever order the rig is given in; nothing of the tick's state is
touched; a sensor follows write_state at once and stays on the body it named when bodies are added; the launch counts are the header's.
No test hands the device call a host pointer, a short buffer or overlapping arrays: those refusals are read in the source
(tests/test_world_batch_sensors_host.py)."""
import numpy as np
import pytest

from tests import batch_query_device_cases as QD
from tests import batch_sensor_cases as SC

pytestmark = pytest.mark.gpu
MASKS = (7, 1, 2, 3, 4)


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


def _reference(b, rig, kinds):
    """(hits, particle rows) by the definition: the restatement's particles from state(), through raycast"""
    from mgf_amd._capi import PARTICLE_DTYPE
    P, D, dt = SC.rig_particles(rig, b.state(), _lengths(b))
    parts = np.zeros(len(rig), PARTICLE_DTYPE)
    parts["p"], parts["d"], parts["dt"] = P, D, dt
    return b.raycast(rig["world"], P, D, dt, ignore=SC.ignore_of(rig), kinds=kinds), parts


def _cast_dev(b, kinds, parts=True):
    """cast_sensors_dev between two waits for the whole device; `out` and `parts` start as 0x5A bytes: a record the call does not write
    shows"""
    import torch
    from mgf_amd._capi import PARTICLE_DTYPE, RAY_HIT_DTYPE
    n = b.sensor_count()
    out = torch.full((n, 7), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    pt = torch.full((n, 7), 0x5A5A5A5A, dtype=torch.int32, device="cuda").view(torch.float32) if parts else None
    _sync()
    b.cast_sensors_dev(out, kinds=kinds, parts=pt)
    _sync()
    return out.cpu().numpy().view(RAY_HIT_DTYPE).reshape(n), (pt.cpu().numpy().view(PARTICLE_DTYPE).reshape(n) if parts else None)


def _assert_casts(b, rig, kinds, want, want_parts, note, repeats=1):
    for rep in range(repeats):
        got, parts = b.cast_sensors(kinds, parts=True)
        assert parts.tobytes() == want_parts.tobytes(), (note, kinds, rep, "particles, host form")
        assert got.tobytes() == want.tobytes(), (note, kinds, rep, "host form", np.flatnonzero(got != want)[:8])
        assert b.cast_sensors(kinds).tobytes() == want.tobytes(), (note, kinds, rep, "host form without particles")
        got, parts = _cast_dev(b, kinds)
        assert parts.tobytes() == want_parts.tobytes(), (note, kinds, rep, "particles, device form")
        assert got.tobytes() == want.tobytes(), (note, kinds, rep, "device form", np.flatnonzero(got != want)[:8])
        got, _ = _cast_dev(b, kinds, parts=False)
        assert got.tobytes() == want.tobytes(), (note, kinds, rep, "device form without particles")


def _spin(b, lay, seed):
    """angular velocities for the bodies that carry a sensor (their linear ones kept)"""
    key = np.unique(lay["world"].astype(np.int64) * 4096 + lay["body"])
    w, bd = (key // 4096).astype(np.int32), (key % 4096).astype(np.int32)
    om = np.random.default_rng(seed).uniform(-9.0, 9.0, (len(w), 3)).astype(np.float32)
    b.set_velocities(w, bd, b.get(w, bd)["linear"], om)
    return w, bd


def _assert_turned(b, w, bd):
    q = b.state()["q"][SC.offsets(_lengths(b))[w] + bd]
    away = np.sum(q != np.float32([1, 0, 0, 0]), axis=1) >= 2
    assert 2 * int(np.sum(away)) >= len(w), (int(np.sum(away)), len(w))     # a rig on unrotated bodies tests nothing of rotate


def _make(ctx, scs, own_terrain):
    import mgf_amd
    return mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=own_terrain)


def _step(b, scs, n=1):
    b.step(float(scs[0]["dt"]), scs[0]["iters"], n)


def _guard(want):
    """the reference meets nothing, bodies, terrain and obstacles, at least eight times each: a condition of the tests, not a measurement"""
    kinds = want["kind"]
    assert set(kinds.tolist()) == {-1, 0, 1, 2}, sorted(set(kinds.tolist()))
    counts = {k: int(np.sum(kinds == k)) for k in (-1, 0, 1, 2)}
    print("reference kinds under QUERY_ALL:", counts)
    assert min(counts.values()) >= 8, counts


def _special(rig, lay, want):
    """the sensor without a direction and the one that is too short meet nothing; of the pair at their body's centre the one that may see
    its own body reports it, at t = 0, and the other does not"""
    role = lay["role"]
    for r in (SC.ZERO, SC.SHORT):
        assert np.all(want["kind"][role == r] == -1), r
    seen, ign = np.flatnonzero(role == SC.SELF_SEEN)[0], np.flatnonzero(role == SC.SELF_IGNORED)[0]
    assert want["kind"][seen] == 0 and want["index"][seen] == rig["body"][seen] and want["t"][seen] == 0.0
    assert not (want["kind"][ign] == 0 and want["index"][ign] == rig["body"][ign])
    for r, kind in ((SC.DOWN, 1), (SC.RING, 2)):                   # aimed at the floor and at the ring
        assert np.mean(want["kind"][role == r] == kind) >= 0.75, (r, want["kind"][role == r])
    assert set(want["kind"][role == SC.UP].tolist()) <= {-1, 2} and np.any(want["kind"][role == SC.UP] == -1)   # the sky, or the ring on the way


CASES = {"twin": (SC.twin_scenes, SC.twin_layout, True), "pile": (QD.pile_scenes, SC.pile_layout, False)}


@pytest.fixture(scope="module", params=sorted(CASES))
def turned(request, ctx):
    """a batch whose sensor bodies have turned for three ticks, its rig aimed from that state and set, and the references under every
    mask - and, taken on the way there, the equality before any tick"""
    scenes, layout, own = CASES[request.param]
    scs = scenes()
    lay = layout(scs)
    b = _make(ctx, scs, own)
    assert b.sensor_count() == 0
    # before any tick: the batch still in its host mirror, the colliders as the bodies were added
    rig0 = SC.aimed_rig(lay, scs, b.state(), _lengths(b))
    b.set_sensors(rig0)
    assert b.sensor_count() == len(rig0)
    for m in MASKS:
        want, want_parts = _reference(b, rig0, m)
        _assert_casts(b, rig0, m, want, want_parts, request.param + " before any tick")
    w, bd = _spin(b, lay, seed=5)
    _step(b, scs, SC.TICKS)
    _assert_turned(b, w, bd)
    rig = SC.aimed_rig(lay, scs, b.state(), _lengths(b))
    b.set_sensors(rig)
    ref = {m: _reference(b, rig, m) for m in MASKS}
    _guard(ref[7][0])
    _special(rig, lay, ref[7][0])
    return dict(name=request.param, b=b, scs=scs, lay=lay, rig=rig, ref=ref, own=own)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_hits_and_particles_equal_the_definition_byte_for_byte(turned):
    b, rig, ref = turned["b"], turned["rig"], turned["ref"]
    for m in MASKS:
        _assert_casts(b, rig, m, ref[m][0], ref[m][1], turned["name"] + " after three ticks", repeats=3)
    assert set(ref[1][0]["kind"].tolist()) == {-1, 0} and set(ref[2][0]["kind"].tolist()) == {-1, 1} and set(ref[4][0]["kind"].tolist()) == {-1, 2}
    # the rig given in reversed order: the same answers, sensor by sensor
    b.set_sensors(rig[::-1].copy())
    for m in MASKS:
        _assert_casts(b, rig[::-1], m, ref[m][0][::-1].copy(), ref[m][1][::-1].copy(), turned["name"] + " reversed")
    # through the arrays of set_sensors too (what the SENSOR_DTYPE form is built from)
    b.set_sensors(rig["world"], rig["body"], rig["p"], rig["d"], rig["dt"], (rig["flags"] & 1).astype(bool))
    _assert_casts(b, rig, 7, ref[7][0], ref[7][1], turned["name"] + " by arrays")


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def _everything(b):
    st = b.state()
    return [st[k].tobytes() for k in ("x", "q", "v", "omega", "delta")] + [b.constraints(k).tobytes() for k in range(b.n_worlds)]


def test_a_step_after_a_cast_is_bit_identical_to_the_twins_step_without_one(ctx):
    scs = SC.twin_scenes()
    lay = SC.twin_layout(scs)
    a, b = _make(ctx, scs, True), _make(ctx, scs, True)
    for t in (a, b):
        _spin(t, lay, seed=6)
        _step(t, scs, SC.TICKS)
    assert _everything(a) == _everything(b)
    b.set_sensors(SC.aimed_rig(lay, scs, b.state(), _lengths(b)))
    for m in (7, 3):
        b.cast_sensors(m, parts=True)
        _cast_dev(b, m)
    assert _everything(a) == _everything(b)          # (a cast writes nothing a reader of the state sees)
    _step(a, scs)
    _step(b, scs)
    _cast_dev(b, 7)
    assert _everything(a) == _everything(b)
    _step(a, scs, 2)
    _step(b, scs, 2)
    assert _everything(a) == _everything(b)


# ---- 3, 4: these change the batch, so each has one of its own -------------------------------------------------------------------------------
def _turned_twin(ctx):
    scs = SC.twin_scenes()
    lay = SC.twin_layout(scs)
    b = _make(ctx, scs, True)
    _spin(b, lay, seed=5)
    _step(b, scs, SC.TICKS)
    rig = SC.aimed_rig(lay, scs, b.state(), _lengths(b))
    b.set_sensors(rig)
    return b, rig, scs


def test_a_sensor_follows_write_state_at_once(ctx):
    b, rig, scs = _turned_twin(ctx)
    k = SC.TWIN_RING_WORLD
    st = b.state(k)
    rng = np.random.default_rng(8)
    q = rng.normal(0, 1, st["q"].shape)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    x = (st["x"] + rng.uniform(-0.2, 0.2, st["x"].shape)).astype(np.float32)
    before = b.cast_sensors(7)
    b.write_state(k, x=x, q=q)
    want, want_parts = _reference(b, rig, 7)      # (state() is the new one; the colliders raycast sees have not moved)
    assert np.array_equal(b.state(k)["q"], q) and want.tobytes() != before.tobytes()
    _assert_casts(b, rig, 7, want, want_parts, "behind write_state")
    _step(b, scs)                                 # and behind the next tick, which moves the colliders
    want, want_parts = _reference(b, rig, 7)
    _assert_casts(b, rig, 7, want, want_parts, "a tick behind write_state")


def test_bodies_added_to_the_middle_world_leave_every_sensor_on_its_body(ctx):
    b, rig, scs = _turned_twin(ctx)
    old = SC.offsets(_lengths(b))
    mid = scs[1]
    comps = mid["comps"][:1].repeat(2)
    comps["p"] += np.float32([[0.0, 1.5, 0.0], [0.0, 3.0, 0.0]])
    b.add_bodies(1, comps, 1.0, float(mid["restitution"][0]), float(mid["friction"][0]), mid["force"][:1].repeat(2, axis=0))
    assert _lengths(b) == [5, 3, 300] and b.sensor_count() == len(rig)
    assert np.any(SC.offsets(_lengths(b))[rig["world"]] != old[rig["world"]])      # flat indices have moved under the rig
    want, want_parts = _reference(b, rig, 7)      # the reference names the same (world, body)
    _assert_casts(b, rig, 7, want, want_parts, "behind add_bodies")
    _step(b, scs)
    want, want_parts = _reference(b, rig, 7)
    _assert_casts(b, rig, 7, want, want_parts, "a tick behind add_bodies", repeats=2)
    assert np.any(want["kind"] >= 0)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_counters_refusals_and_the_empty_rig(ctx):
    import mgf_amd
    from mgf_amd import _capi
    for scenes, layout, own, K in ((SC.twin_scenes, SC.twin_layout, True, 3), (QD.pile_scenes, SC.pile_layout, False, 5)):
        scs = scenes()
        b = _make(ctx, scs, own)
        assert b.n_worlds == K
        lay = layout(scs)
        full = SC.aimed_rig(lay, scs, b.state(), _lengths(b))
        big = np.resize(full, 600)
        launches = {}
        for name, rig in (("one", full[:1]), ("all", full), ("600", big)):
            b.set_sensors(rig.copy())
            assert b.sensor_count() == len(rig)
            skipped = b.counter("device_skipped")
            got = []
            for m in (7, 3):                                   # with and without the obstacle pass (a world of each batch has a ring)
                b.cast_sensors(m)
                got.append(b.counter("query_launches"))
                _cast_dev(b, m)
                got.append(b.counter("query_launches"))
            launches[name] = got
            assert b.counter("device_skipped") == skipped
        assert launches["one"] == launches["all"] == launches["600"] == [_capi.BATCH_SENSOR_LAUNCHES + 1] * 2 + [_capi.BATCH_SENSOR_LAUNCHES] * 2, launches
        _step(b, scs)
        _cast_dev(b, 7)
        assert b.counter("query_launches") == _capi.BATCH_SENSOR_LAUNCHES + 1 + 1      # the collider gather behind a step, once
        _cast_dev(b, 7)
        assert b.counter("query_launches") == _capi.BATCH_SENSOR_LAUNCHES + 1
        _step(b, scs)
        b.cast_sensors(2)
        assert b.counter("query_launches") == _capi.BATCH_SENSOR_LAUNCHES + 1
        b.cast_sensors(2)
        assert b.counter("query_launches") == _capi.BATCH_SENSOR_LAUNCHES
        # refused on the host, the rig as it was
        n = b.sensor_count()
        kept = b.cast_sensors(7)
        lens = _lengths(b)
        for field, value in (("world", -1), ("world", K), ("body", -1), ("body", lens[int(big["world"][5])]), ("flags", 2), ("flags", 3), ("flags", -1)):
            bad = big.copy()
            bad[field][5] = value
            with pytest.raises(mgf_amd.MgfError) as e:
                b.set_sensors(bad)
            assert e.value.status == _capi.ERR_INVALID and b.sensor_count() == n, (field, value)
        lib = mgf_amd.load_library()
        out = np.zeros(n, _capi.RAY_HIT_DTYPE)
        assert lib.mgf_batch_cast_sensors(b._h, 7, out.ctypes.data, None, n - 1) == _capi.ERR_CAPACITY
        assert lib.mgf_batch_cast_sensors(b._h, 7, None, None, n) == _capi.ERR_INVALID          # (a rig that is not empty needs somewhere to go)
        assert lib.mgf_batch_cast_sensors_dev(b._h, 7, None, None, n) == _capi.ERR_INVALID
        import torch
        dev = torch.zeros((n, 7), dtype=torch.int32, device="cuda")
        _sync()
        assert lib.mgf_batch_cast_sensors_dev(b._h, 7, dev.data_ptr(), None, n - 1) == _capi.ERR_CAPACITY
        assert b.sensor_count() == n and b.cast_sensors(7).tobytes() == kept.tobytes()
        # n = 0 empties the rig; a cast then enqueues nothing
        b.set_sensors(np.zeros(0, _capi.SENSOR_DTYPE))
        assert b.sensor_count() == 0
        assert len(b.cast_sensors(7)) == 0 and b.counter("query_launches") == 0
        hits, parts = b.cast_sensors(7, parts=True)
        assert len(hits) == 0 and len(parts) == 0
        empty = torch.zeros((0, 7), dtype=torch.int32, device="cuda")
        b.cast_sensors_dev(empty)
        assert b.counter("query_launches") == 0
        del b
