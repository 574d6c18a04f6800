"""The body-mounted depth cameras of a batch (mgf_batch_set_cameras / _cast_cameras / _cast_cameras_dev; WorldBatch.set_cameras /
.cast_cameras / .cast_cameras_dev) against their definition on the SAME batch at the same moment: every pixel's particle equals the
numpy restatement (tests/batch_camera_cases.py) over state() byte for byte, every pixel's hit equals raycast of that particle byte for
byte and its depth is that hit's t, or far - under every mask, before a tick and after three, on bodies that have turned; the images
equal cast_sensors of a rig with one sensor a pixel; the device form equals the host form for every combination of outputs; nothing of
the tick's state is touched; a camera follows write_state at once and stays on its body when bodies are added; the camera rig and the
sensor rig do not see each other; the launch counts are the header's.  Every pixel is compared: no tolerance, no sample.
The scenes are tests/batch_camera_cases.camera_scenes(), of which tests/test_world_batch_cameras_host.py shows with the oracle's ray
tests that they hold bodies, terrain, obstacles and nothing, tiles whose cone leaves bodies out that other tiles hit, an eye inside a
body and bodies beyond far: here the same kinds are found again, camera by camera, before any tick."""
import itertools

import numpy as np
import pytest

from tests import batch_camera_cases as CC
from tests import batch_sensor_cases as SC

pytestmark = pytest.mark.gpu
MASKS = (7, 1, 2, 4, 3)


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
    """(depth, hits, particle rows) by the definition: the restatement's particles from state(), through raycast"""
    from mgf_amd._capi import PARTICLE_DTYPE
    W, P, D, T, I = CC.rig_particles(rig, b.state(), _lengths(b))
    parts = np.zeros(len(W), PARTICLE_DTYPE)
    parts["p"], parts["d"], parts["dt"] = P, D, T
    hits = b.raycast(W, P, D, T, ignore=I, kinds=kinds)
    depth = np.where(hits["kind"] == -1, T, hits["t"]).astype(np.float32)
    return depth, hits, parts


def _flat(images):
    return np.concatenate([im.ravel() for im in images]) if images else np.zeros(0, np.float32)


def _cast_dev(b, kinds, depth=True, hits=True, parts=True):
    """cast_cameras_dev between two waits for the whole device; every array starts as 0x5A bytes: a record the call does not write shows"""
    import torch
    from mgf_amd._capi import PARTICLE_DTYPE, RAY_HIT_DTYPE
    n = b.camera_pixels()
    fill = lambda *shape: torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d = fill(n).view(torch.float32) if depth else None
    h = fill(n, 7) if hits else None
    p = fill(n, 7).view(torch.float32) if parts else None
    _sync()
    b.cast_cameras_dev(depth=d, hits=h, parts=p, kinds=kinds)
    _sync()
    return (d.cpu().numpy() if depth else None, h.cpu().numpy().view(RAY_HIT_DTYPE).reshape(n) if hits else None,
            p.cpu().numpy().view(PARTICLE_DTYPE).reshape(n) if parts else None)


def _assert_casts(b, kinds, want, note, repeats=1):
    wd, wh, wp = want
    for rep in range(repeats):
        images, hits, parts = b.cast_cameras(kinds, hits=True, parts=True)
        assert parts.tobytes() == wp.tobytes(), (note, kinds, rep, "particles, host form", np.flatnonzero(parts != wp)[:8])
        assert hits.tobytes() == wh.tobytes(), (note, kinds, rep, "hits, host form", np.flatnonzero(hits != wh)[:8])
        assert _flat(images).tobytes() == wd.tobytes(), (note, kinds, rep, "depth, host form")
        assert _flat(b.cast_cameras(kinds)).tobytes() == wd.tobytes(), (note, kinds, rep, "depth alone, host form")
        d, h, p = _cast_dev(b, kinds)
        assert p.tobytes() == wp.tobytes(), (note, kinds, rep, "particles, device form")
        assert h.tobytes() == wh.tobytes(), (note, kinds, rep, "hits, device form", np.flatnonzero(h != wh)[:8])
        assert d.tobytes() == wd.tobytes(), (note, kinds, rep, "depth, device form")


def _spin(b, rig, seed):
    """angular velocities for the bodies that carry a camera (their linear ones kept)"""
    key = np.unique(rig["world"].astype(np.int64) * 4096 + rig["body"])
    w, bd = (key // 4096).astype(np.int32), (key % 4096).astype(np.int32)
    om = np.random.default_rng(seed).uniform(-9.0, 9.0, (len(w), 3)).astype(np.float32)
    b.set_velocities(w, bd, b.get(w, bd)["linear"], om)
    return w, bd


def _make(ctx, scs):
    import mgf_amd
    return mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)


def _step(b, scs, n=1):
    b.step(float(scs[0]["dt"]), scs[0]["iters"], n)


def _turned(ctx, seed=5):
    scs, _ = CC.camera_scenes()
    rig = CC.camera_rig(scs)
    b = _make(ctx, scs)
    w, bd = _spin(b, rig, seed)
    _step(b, scs, CC.TICKS)
    q = b.state()["q"][SC.offsets(_lengths(b))[w] + bd]
    assert 2 * int(np.sum(np.sum(q != np.float32([1, 0, 0, 0]), axis=1) >= 2)) >= len(w)     # a rig on unrotated bodies tests nothing of rotate
    b.set_cameras(rig)
    return b, rig, scs


@pytest.fixture(scope="module")
def turned(ctx):
    """a batch whose camera bodies have turned for three ticks and the references under every mask - and, taken on the way there, the
    equality before any tick, where the scenes are what tests/test_world_batch_cameras_host.py looked at"""
    scs, long_body = CC.camera_scenes()
    rig = CC.camera_rig(scs)
    b = _make(ctx, scs)
    assert b.camera_count() == 0 and b.camera_pixels() == 0
    st, first = b.state(), CC.initial_state(scs)
    g = SC.offsets(_lengths(b))[rig["world"]] + rig["body"]
    assert np.array_equal(st["x"][g], first["x"][g]) and np.array_equal(st["q"][g], first["q"][g])     # what the check without a GPU took for granted
    b.set_cameras(rig)
    assert b.camera_count() == len(rig) and b.camera_pixels() == CC.camera_pixels(rig)
    fs = CC.firsts(rig)
    for m in MASKS:
        want = _reference(b, rig, m)
        _assert_casts(b, m, want, "before any tick")
        if m == 7:
            for c, name in enumerate(CC.NAMES):
                n = int(rig["width"][c]) * int(rig["height"][c])
                assert set(want[1]["kind"][fs[c]:fs[c] + n].tolist()) == CC.SEES[name], name
            above = want[1][:64 * 64]
            assert np.sum((above["kind"] == 0) & (above["index"] == long_body)) >= 100               # the long capsule, across the image
    w, bd = _spin(b, rig, seed=5)
    _step(b, scs, CC.TICKS)
    ref = {m: _reference(b, rig, m) for m in MASKS}
    kinds = ref[7][1]["kind"]
    counts = {k: int(np.sum(kinds == k)) for k in (-1, 0, 1, 2)}
    print("reference kinds under QUERY_ALL after three ticks:", counts)
    assert min(counts.values()) >= 8, counts
    return dict(b=b, scs=scs, rig=rig, ref=ref)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_depth_hits_and_particles_equal_the_definition_byte_for_byte(turned):
    b, rig, ref = turned["b"], turned["rig"], turned["ref"]
    for m in MASKS:
        _assert_casts(b, m, ref[m], "after three ticks", repeats=2)
        d, h, p = ref[m]
        assert np.array_equal(d[h["kind"] >= 0], h["t"][h["kind"] >= 0]) and np.array_equal(d[h["kind"] < 0], p["dt"][h["kind"] < 0])
    assert set(ref[1][1]["kind"].tolist()) == {-1, 0} and set(ref[2][1]["kind"].tolist()) == {-1, 1} and set(ref[4][1]["kind"].tolist()) == {-1, 2}
    # the images have the cameras' shapes, row 0 at the top
    images = b.cast_cameras(7)
    assert [im.shape for im in images] == [(int(h), int(w)) for h, w in zip(rig["height"], rig["width"])] and all(im.dtype == np.float32 for im in images)
    # the rig given in reversed order: the same images, camera by camera
    b.set_cameras(rig[::-1].copy())
    back = b.cast_cameras(7)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(back[::-1], images))
    # through dicts too
    b.set_cameras([{k: rig[k][i] for k in rig.dtype.names} for i in range(len(rig))])
    _assert_casts(b, 7, ref[7], "by dicts")


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_cameras_equal_a_sensor_rig_of_one_sensor_a_pixel_and_the_rigs_do_not_see_each_other(turned):
    from mgf_amd._capi import SENSOR_DTYPE
    b, rig, ref = turned["b"], turned["rig"], turned["ref"]
    b.set_cameras(rig)
    assert b.sensor_count() == 0
    sensors = CC.sensor_rig(rig)
    assert len(sensors) == b.camera_pixels()
    b.set_sensors(sensors)
    assert b.camera_count() == len(rig)
    for m in MASKS:
        hits, parts = b.cast_sensors(m, parts=True)
        assert parts.tobytes() == ref[m][2].tobytes() and hits.tobytes() == ref[m][1].tobytes(), m
        _assert_casts(b, m, ref[m], "with a sensor rig set")          # ... and the cameras are as they were
    want_sensors = b.cast_sensors(7)
    b.set_cameras(rig[:2].copy())                                     # the camera rig changed, then cleared: the sensors' answers stay
    assert b.cast_sensors(7).tobytes() == want_sensors.tobytes()
    b.set_cameras(np.zeros(0, rig.dtype))
    assert b.camera_count() == 0 and b.sensor_count() == len(sensors) and b.cast_sensors(7).tobytes() == want_sensors.tobytes()
    b.set_cameras(rig)
    b.set_sensors(sensors[:5].copy())                                 # the sensor rig changed, then cleared: the cameras' answers stay
    _assert_casts(b, 7, ref[7], "with another sensor rig")
    b.set_sensors(np.zeros(0, SENSOR_DTYPE))
    assert b.sensor_count() == 0 and b.camera_count() == len(rig)
    _assert_casts(b, 7, ref[7], "with the sensor rig cleared")


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_device_form_equals_the_host_form_for_every_combination_of_outputs(turned):
    b, rig, ref = turned["b"], turned["rig"], turned["ref"]
    b.set_cameras(rig)
    for m in (7, 3):                                                  # with and without the obstacle pass
        images, hits, parts = b.cast_cameras(m, hits=True, parts=True)
        assert _flat(images).tobytes() == ref[m][0].tobytes()
        for depth, want_hits, want_parts in itertools.product((True, False), repeat=3):
            if not depth and not want_hits:
                continue
            d, h, p = _cast_dev(b, m, depth, want_hits, want_parts)
            note = (m, depth, want_hits, want_parts)
            assert (d is None) == (not depth) and (h is None) == (not want_hits) and (p is None) == (not want_parts)
            if depth:
                assert d.tobytes() == _flat(images).tobytes(), note
            if want_hits:
                assert h.tobytes() == hits.tobytes(), note
            if want_parts:
                assert p.tobytes() == parts.tobytes(), note
        images2, hits2 = b.cast_cameras(m, hits=True)                 # the host form's own combinations
        assert _flat(images2).tobytes() == _flat(images).tobytes() and hits2.tobytes() == hits.tobytes()
        images3, parts3 = b.cast_cameras(m, parts=True)
        assert _flat(images3).tobytes() == _flat(images).tobytes() and parts3.tobytes() == parts.tobytes()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def _everything(b):
    st = b.state()
    return [st[k].tobytes() for k in ("x", "q", "v", "omega", "delta")] + [b.constraints(k).tobytes() for k in range(b.n_worlds)]


def test_a_step_after_a_cast_is_bit_identical_to_the_twins_step_without_one(ctx):
    scs, _ = CC.camera_scenes()
    rig = CC.camera_rig(scs)
    a, b = _make(ctx, scs), _make(ctx, scs)
    for t in (a, b):
        _spin(t, rig, seed=6)
        _step(t, scs, CC.TICKS)
    assert _everything(a) == _everything(b)
    b.set_cameras(rig)
    for m in (7, 3):
        b.cast_cameras(m, hits=True, parts=True)
        _cast_dev(b, m)
    assert _everything(a) == _everything(b)          # (a cast writes nothing a reader of the state sees)
    _step(a, scs)
    _step(b, scs)
    _cast_dev(b, 7)
    assert _everything(a) == _everything(b)
    _step(a, scs, 2)
    _step(b, scs, 2)
    assert _everything(a) == _everything(b)


# ---- 5: these change the batch, so each has one of its own ----------------------------------------------------------------------------------
def test_a_camera_follows_write_state_at_once(ctx):
    b, rig, scs = _turned(ctx)
    k = CC.CAMERA_WORLD
    st = b.state(k)
    rng = np.random.default_rng(8)
    q = rng.normal(0, 1, st["q"].shape)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    x = (st["x"] + rng.uniform(-0.2, 0.2, st["x"].shape)).astype(np.float32)
    before = _flat(b.cast_cameras(7))
    b.write_state(k, x=x, q=q)
    want = _reference(b, rig, 7)                  # (state() is the new one; the colliders raycast sees have not moved)
    assert np.array_equal(b.state(k)["q"], q) and want[0].tobytes() != before.tobytes()
    _assert_casts(b, 7, want, "behind write_state")
    _step(b, scs)                                 # and behind the next tick, which moves the colliders
    _assert_casts(b, 7, _reference(b, rig, 7), "a tick behind write_state")


def test_bodies_added_to_the_middle_world_leave_every_camera_on_its_body(ctx):
    b, rig, scs = _turned(ctx)
    old = SC.offsets(_lengths(b))
    mid = scs[1]
    comps = mid["comps"][:1].repeat(2)
    comps["p"] += np.float32([[0.0, 1.5, 0.0], [0.0, 3.0, 0.0]])
    b.add_bodies(1, comps, 1.0, float(mid["restitution"][0]), float(mid["friction"][0]), mid["force"][:1].repeat(2, axis=0))
    assert _lengths(b) == [5, 3, 300] and b.camera_count() == len(rig) and b.camera_pixels() == CC.camera_pixels(rig)
    assert np.any(SC.offsets(_lengths(b))[rig["world"]] != old[rig["world"]])      # flat indices have moved under the rig
    _assert_casts(b, 7, _reference(b, rig, 7), "behind add_bodies")                # the reference names the same (world, body)
    _step(b, scs)
    want = _reference(b, rig, 7)
    _assert_casts(b, 7, want, "a tick behind add_bodies", repeats=2)
    assert np.any(want[1]["kind"] >= 0)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_counters_refusals_and_the_empty_rig(ctx):
    import torch
    import mgf_amd
    from mgf_amd import _capi
    scs, _ = CC.camera_scenes()
    full = CC.camera_rig(scs)
    b = _make(ctx, scs)
    one = full[4:5].copy()                                       # a camera of one pixel
    many = np.concatenate([full, full, full])
    launches = {}
    for name, rig in (("one", one), ("all", full), ("many", many)):
        b.set_cameras(rig.copy())
        assert b.camera_count() == len(rig) and b.camera_pixels() == CC.camera_pixels(rig)
        skipped = b.counter("device_skipped")
        got = []
        for m in (7, 3):                                         # with and without the obstacle pass (a world of the batch has a ring)
            b.cast_cameras(m)
            got.append(b.counter("query_launches"))
            _cast_dev(b, m)
            got.append(b.counter("query_launches"))
            _cast_dev(b, m, depth=False)                         # hits alone: no depth pass
            got.append(b.counter("query_launches"))
        launches[name] = got
        assert b.counter("device_skipped") == skipped
    L = _capi.BATCH_CAMERA_LAUNCHES
    assert L == 1 and launches["one"] == launches["all"] == launches["many"] == [L + 2, L + 2, L + 1, L, L, L], launches
    b.set_cameras(full)
    _step(b, scs)
    _cast_dev(b, 7)
    assert b.counter("query_launches") == 3 + 1                  # the collider gather behind a step, once
    _cast_dev(b, 7)
    assert b.counter("query_launches") == 3
    _step(b, scs)
    b.cast_cameras(2)
    assert b.counter("query_launches") == 1 + 1
    b.cast_cameras(2)
    assert b.counter("query_launches") == 1
    # refused on the host, the rig as it was
    n, pixels = b.camera_count(), b.camera_pixels()
    kept = _flat(b.cast_cameras(7))
    lens = _lengths(b)
    K = b.n_worlds
    bad_values = [("world", -1), ("world", K), ("body", -1), ("body", lens[int(full["world"][1])]), ("flags", 2), ("flags", 3), ("flags", -1), ("reserved", 1),
                  ("width", 0), ("width", -3), ("width", 4097), ("height", 0), ("height", 4097), ("tan_x", np.inf), ("tan_y", np.nan), ("far", 0.0),
                  ("far", -1.0), ("far", np.nan), ("far", -np.inf)]
    for field, value in bad_values:
        bad = full.copy()
        bad[field][1] = value
        with pytest.raises(mgf_amd.MgfError) as e:
            b.set_cameras(bad)
        assert e.value.status == _capi.ERR_INVALID and b.camera_count() == n and b.camera_pixels() == pixels, (field, value)
    for field, at, value in (("p", 2, np.nan), ("p", 0, np.inf), ("r", 0, np.nan), ("r", 3, -np.inf)):
        bad = full.copy()
        bad[field][1, at] = value
        with pytest.raises(mgf_amd.MgfError) as e:
            b.set_cameras(bad)
        assert e.value.status == _capi.ERR_INVALID and b.camera_count() == n, (field, at)
    huge = np.repeat(full[:1], 129)                              # 128 images of 4096 x 4096 are 2^31 pixels
    huge["width"], huge["height"] = 4096, 4096
    with pytest.raises(mgf_amd.MgfError) as e:
        b.set_cameras(huge)
    assert e.value.status == _capi.ERR_INVALID and "INT32_MAX" in str(e.value) and b.camera_pixels() == pixels
    ok = full.copy()
    ok["far"][1], ok["width"][4], ok["height"][4] = np.inf, 4096, 1     # what is NOT refused: far = +inf, a side of 4096
    b.set_cameras(ok)
    assert b.camera_pixels() == pixels + 4095
    _assert_casts(b, 7, _reference(b, ok, 7), "a camera of 4096 x 1")
    b.set_cameras(full)
    lib = mgf_amd.load_library()
    depth, out = np.zeros(pixels, np.float32), np.zeros(pixels, _capi.RAY_HIT_DTYPE)
    assert lib.mgf_batch_cast_cameras(b._h, 7, depth.ctypes.data, out.ctypes.data, None, pixels - 1) == _capi.ERR_CAPACITY
    assert lib.mgf_batch_cast_cameras(b._h, 7, None, None, None, pixels) == _capi.ERR_INVALID          # (a rig that is not empty needs somewhere to go)
    assert lib.mgf_batch_cast_cameras_dev(b._h, 7, None, None, None, pixels) == _capi.ERR_INVALID
    dev = torch.zeros(pixels, dtype=torch.float32, device="cuda")
    _sync()
    assert lib.mgf_batch_cast_cameras_dev(b._h, 7, dev.data_ptr(), None, None, pixels - 1) == _capi.ERR_CAPACITY
    assert lib.mgf_batch_cast_cameras(b._h, 7, None, out.ctypes.data, None, pixels) == _capi.OK      # hits alone will do
    assert b.camera_count() == n and _flat(b.cast_cameras(7)).tobytes() == kept.tobytes()
    # n = 0 empties the rig; a cast then enqueues nothing
    b.set_cameras(np.zeros(0, _capi.CAMERA_DTYPE))
    assert b.camera_count() == 0 and b.camera_pixels() == 0
    assert b.cast_cameras(7) == [] and b.counter("query_launches") == 0
    images, hits, parts = b.cast_cameras(7, hits=True, parts=True)
    assert images == [] and len(hits) == 0 and len(parts) == 0
    b.cast_cameras_dev(depth=torch.zeros(0, dtype=torch.float32, device="cuda"))
    assert b.counter("query_launches") == 0
    assert lib.mgf_batch_cast_cameras(b._h, 7, None, None, None, 0) == _capi.OK
    del b
