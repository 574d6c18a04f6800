"""The body-mounted actuators of a batch (mgf_batch_set_actuators / _actuate / _actuate_dev; WorldBatch.set_actuators / .actuate /
.actuate_dev) against their definition, on twin batches built from the same scenes and ticked until the bodies have turned: the
wrenches equal the numpy restatement over state() bit for bit (tests/batch_actuator_cases.py, held to the oracle by
tests/test_world_batch_actuators_host.py); the impulse mode leaves the batch bit for bit as apply_impulses of those wrenches leaves its
twin, the force mode as get, the restated sequential adds and set_forces leave it, now and ticks later; worlds no actuator names equal
an untouched third twin; the device form equals the host form, costs one launch and counts the planted non-finite controls; the rig
stays on the bodies it named when bodies are added; write_state turns the next wrench at once; what needs the handle is refused with
the rig and the state as they were."""
import numpy as np
import pytest

from tests import batch_actuator_cases as AC
from tests import batch_drive_cases as DC

pytestmark = pytest.mark.gpu
IMPULSE, FORCE = AC.IMPULSE, AC.FORCE


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


def _all(b):
    lens = _lengths(b)
    return (np.concatenate([np.full(n, k, np.int32) for k, n in enumerate(lens)]), np.concatenate([np.arange(n, dtype=np.int32) for n in lens]))


def _step(b, scs, n=1):
    b.step(float(scs[0]["dt"]), scs[0]["iters"], n)


def _everything(b, worlds=None):
    """what a caller can read of the bodies: state() and get() of every body (of the given worlds), as bytes"""
    w, bd = _all(b)
    st = b.state()
    got = b.get(w, bd)
    keep = np.ones(len(w), bool) if worlds is None else np.isin(w, worlds)
    return [st[k][keep].tobytes() for k in DC.STATE] + [got[keep].tobytes()]


def _twins(ctx, count, seed=7, late=True):
    """`count` batches of AC.actuator_scenes(), spun, ticked until the bodies have turned, then - late - two bodies added to
    LATE_WORLD: bodies no tick has touched"""
    import mgf_amd
    scs = AC.actuator_scenes()
    out = []
    for _ in range(count):
        b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
        w, bd = _all(b)
        om = np.random.default_rng(seed).uniform(-9.0, 9.0, (len(w), 3)).astype(np.float32)
        b.set_velocities(w, bd, b.get(w, bd)["linear"], om)
        _step(b, scs, AC.TICKS)
        if late:
            b.add_bodies(AC.LATE_WORLD, *AC.late_bodies(scs[AC.LATE_WORLD]))
        out.append(b)
    q = out[0].state()["q"]
    away = np.sum(q != np.float32([1, 0, 0, 0]), axis=1) >= 2
    assert 2 * int(np.sum(away)) >= len(q), (int(np.sum(away)), len(q))      # a rig on unrotated bodies tests nothing of rotate
    for b in out[1:]:
        assert _everything(b) == _everything(out[0])
    return out, scs


def _where(got, want):
    return [i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()][:8]


def _actuate_dev(b, u, mode, wrenches=True):
    """actuate_dev between two waits for the whole device; the wrench buffer starts as 0x5A bytes: a row the call does not write shows"""
    import torch
    n = b.actuator_count()
    ud = torch.from_numpy(np.ascontiguousarray(u, np.float32)).cuda()
    out = torch.full((n, 6), 0x5A5A5A5A, dtype=torch.int32, device="cuda").view(torch.float32) if wrenches else None
    _sync()
    b.actuate_dev(ud, mode, wrenches_out=out)
    launches = b.counter("drive_launches")
    _sync()
    return (out.cpu().numpy() if wrenches else None), launches


def _force_reference(b, rig, W):
    """the force mode by its definition on a twin: get of the rows, the restated sequential adds, set_forces"""
    before = b.get(rig["world"], rig["body"])
    uw, ub, F, T = AC.forces_expected(before, rig["world"], rig["body"], W)
    b.set_forces(uw, ub, F, T)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_impulse_mode_is_apply_impulses_of_the_restated_wrenches(ctx):
    (a, b, c), scs = _twins(ctx, 3)
    lens = _lengths(a)
    assert lens == [48, 8, 18, 64, 8 + AC.LATE_BODIES]
    rig, u, planted = AC.main_rig(lens)
    assert a.actuator_count() == 0
    a.set_actuators(rig)
    assert a.actuator_count() == len(rig)
    want, skipped = AC.rig_wrenches(rig, u, a.state(), lens)
    W = a.actuate(u, IMPULSE, wrenches=True)
    assert a.counter("drive_launches") == 1
    assert W.dtype == np.float32 and W.shape == (len(rig), 6)
    assert W.tobytes() == want.tobytes(), ("wrenches", _where(W, want))
    assert np.all(W[planted] == 0) and a.counter("actuators_skipped") == len(planted) == int(skipped.sum())
    for fl in range(4):                                                       # every branch gave a wrench that is not zero
        assert np.any(W[(rig["flags"] == fl) & ~skipped] != 0), fl
    b.apply_impulses(rig["world"], rig["body"], W[:, 0:3], W[:, 3:6])
    assert _everything(a) == _everything(b)
    assert _everything(a) != _everything(c)
    bare = [AC.BARE_WORLD]
    assert _everything(a, bare) == _everything(c, bare)                       # a world no actuator names: the untouched twin's
    # the header's arithmetic once more, from get() just before: v = v + L * inv_mass, omega = omega + I * A in the caller's order
    v, om = DC.impulses_expected(c.get(rig["world"], rig["body"]), rig["world"], rig["body"], W[:, 0:3], W[:, 3:6])
    got = a.get(rig["world"], rig["body"])
    assert got["linear"].tobytes() == v.tobytes() and got["angular"].tobytes() == om.tobytes()
    for t in (a, b, c):
        _step(t, scs, 3)
    assert _everything(a) == _everything(b)
    assert _everything(a, bare) == _everything(c, bare)
    assert all(a.constraints(k).tobytes() == b.constraints(k).tobytes() for k in range(a.n_worlds))
    # without the wrenches the call does the same
    want2, _ = AC.rig_wrenches(rig, u, a.state(), lens)
    assert a.actuate(u, IMPULSE) is None
    b.apply_impulses(rig["world"], rig["body"], want2[:, 0:3], want2[:, 3:6])
    assert _everything(a) == _everything(b)
    assert a.counter("actuators_skipped") == 2 * len(planted)                 # cumulative


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_force_mode_adds_to_the_rows_in_the_callers_order_and_accumulates(ctx):
    (a, b, c), scs = _twins(ctx, 3, seed=8)
    lens = _lengths(a)
    rig, u, planted = AC.main_rig(lens)
    a.set_actuators(rig)
    w, bd = _all(a)
    rows0 = a.get(w, bd)
    W = a.actuate(u, FORCE, wrenches=True)
    assert a.counter("drive_launches") == 1
    want, _ = AC.rig_wrenches(rig, u, a.state(), lens)
    assert W.tobytes() == want.tobytes(), _where(W, want)
    _force_reference(b, rig, W)
    rows = a.get(w, bd)
    assert rows["force"].tobytes() == b.get(w, bd)["force"].tobytes() and rows["torque"].tobytes() == b.get(w, bd)["torque"].tobytes()
    assert _everything(a) == _everything(b)
    named = np.zeros(len(w), bool)
    named[AC.SC.offsets(lens)[rig["world"]] + rig["body"]] = True
    assert np.any(rows["force"][named] != rows0["force"][named]) and np.any(rows["torque"][named] != rows0["torque"][named])
    assert rows[~named].tobytes() == rows0[~named].tobytes()                  # velocities and every row of the others as they were
    for k in ("linear", "angular", "x", "inv_mass", "inv_moment"):
        assert rows[k].tobytes() == rows0[k].tobytes(), k
    # a second call accumulates: the rows grow by the same wrenches again (q has not moved)
    W2 = a.actuate(u, FORCE, wrenches=True)
    assert W2.tobytes() == W.tobytes()
    _force_reference(b, rig, W2)
    assert _everything(a) == _everything(b)
    once = np.flatnonzero(np.bincount(AC.SC.offsets(lens)[rig["world"]] + rig["body"], minlength=len(w)) == 1)
    i = {int(AC.SC.offsets(lens)[rig["world"][k]] + rig["body"][k]): k for k in range(len(rig))}
    g = next(int(x) for x in once if np.any(W[i[int(x)], 0:3] != 0))
    assert a.get(w, bd)["force"][g].tobytes() == ((rows0["force"][g] + W[i[g], 0:3]) + W[i[g], 0:3]).astype(np.float32).tobytes()
    # the rows hold for every later tick
    for t in (a, b, c):
        _step(t, scs, 5)
    assert _everything(a) == _everything(b)
    bare = [AC.BARE_WORLD]
    assert _everything(a, bare) == _everything(c, bare) and _everything(a) != _everything(c)
    assert all(a.constraints(k).tobytes() == b.constraints(k).tobytes() for k in range(a.n_worlds))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_device_form_equals_the_host_form_costs_one_launch_and_follows_added_bodies_and_written_poses(ctx):
    (a, b, c), scs = _twins(ctx, 3, seed=9)
    lens = _lengths(a)
    rig, u, planted = AC.main_rig(lens)
    a.set_actuators(rig)
    b.set_actuators(rig)
    for mode in (IMPULSE, FORCE):
        Wd, launches = _actuate_dev(a, u, mode)
        assert launches == 1
        Wh = b.actuate(u, mode, wrenches=True)
        assert b.counter("drive_launches") == 1
        assert Wd.tobytes() == Wh.tobytes(), (mode, _where(Wd, Wh))
        assert _everything(a) == _everything(b), mode
    assert a.counter("actuators_skipped") == 2 * len(planted) == b.counter("actuators_skipped")
    none, launches = _actuate_dev(a, u, IMPULSE, wrenches=False)              # without the wrench buffer
    b.actuate(u, IMPULSE)
    assert none is None and launches == 1 and _everything(a) == _everything(b)
    # one launch for one actuator as for all of them
    c.set_actuators(rig[:1])
    _, launches = _actuate_dev(c, u[:1], IMPULSE)
    assert launches == 1
    c.set_actuators(np.zeros(0, rig.dtype))
    import torch
    c.actuate_dev(torch.zeros(0, dtype=torch.float32, device="cuda"), IMPULSE)
    assert c.counter("drive_launches") == 0 and c.actuator_count() == 0       # an empty rig enqueues nothing
    assert c.actuate(np.zeros(0, np.float32), FORCE, wrenches=True).shape == (0, 6) and c.counter("drive_launches") == 0
    # bodies added to an earlier world between two calls: flat indices move under the rig, every actuator stays on its body
    for t in (a, b):
        _step(t, scs, 2)
        t.add_bodies(AC.BARE_WORLD, *AC.late_bodies(scs[AC.BARE_WORLD]))
    lens2 = _lengths(a)
    assert lens2[AC.BARE_WORLD] == lens[AC.BARE_WORLD] + AC.LATE_BODIES and a.actuator_count() == len(rig)
    want, _ = AC.rig_wrenches(rig, u, a.state(), lens2)
    Wd, launches = _actuate_dev(a, u, IMPULSE)
    assert launches == 1 and Wd.tobytes() == want.tobytes(), _where(Wd, want)
    b.apply_impulses(rig["world"], rig["body"], Wd[:, 0:3], Wd[:, 3:6])
    assert _everything(a) == _everything(b)
    # a pose written with write_state turns the next wrench at once
    k = AC.PILE_WORLD
    st = a.state(k)
    q = st["q"][:, [3, 0, 1, 2]] * np.float32([-1, 1, 1, 1])                  # another unit quaternion per body
    for t in (a, b):
        t.write_state(k, q=q)
    want, _ = AC.rig_wrenches(rig, u, a.state(), lens2)
    here = (rig["world"] == k) & ((rig["flags"] & AC.WORLD_DIR) == 0)
    Wd2, _ = _actuate_dev(a, u, FORCE)
    assert Wd2.tobytes() == want.tobytes(), _where(Wd2, want)
    assert np.any(Wd2[here] != Wd[here]) and Wd2[rig["world"] != k].tobytes() == Wd[rig["world"] != k].tobytes()
    _force_reference(b, rig, Wd2)
    for t in (a, b):
        _step(t, scs)
    assert _everything(a) == _everything(b)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_no_tick_has_touched_and_a_dumbbell(ctx):
    import mgf_amd
    from tests import batch_parts_cases as PC
    # before the first tick: the mirror goes up with the call
    scs = AC.actuator_scenes()
    a, b = (mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True) for _ in range(2))
    lens = _lengths(a)
    rig, u, planted = AC.main_rig([n + (AC.LATE_BODIES if k == AC.LATE_WORLD else 0) for k, n in enumerate(lens)])
    rig["body"][rig["world"] == AC.LATE_WORLD] %= lens[AC.LATE_WORLD]
    a.set_actuators(rig)
    want, _ = AC.rig_wrenches(rig, u, a.state(), lens)
    W = a.actuate(u, IMPULSE, wrenches=True)
    assert W.tobytes() == want.tobytes(), _where(W, want)
    b.apply_impulses(rig["world"], rig["body"], W[:, 0:3], W[:, 3:6])
    assert _everything(a) == _everything(b)
    for t in (a, b):
        _step(t, scs, 2)
    assert _everything(a) == _everything(b)
    # bodies of several components: actuators read no shapes, the batch is answered - on a dumbbell as on a plain sphere
    dsc = [PC.six_scenes()[PC.DUMBBELLS]]
    a, b = (mgf_amd.WorldBatch.from_scenes(ctx, dsc, own_terrain=True) for _ in range(2))
    for t in (a, b):
        _step(t, dsc, 4)
    n = _lengths(a)[0]
    drig, du = AC.dumbbell_rig(n)
    a.set_actuators(drig)
    for mode in (IMPULSE, FORCE):
        want, _ = AC.rig_wrenches(drig, du, a.state(), [n])
        Wd, launches = _actuate_dev(a, du, mode)
        assert launches == 1 and Wd.tobytes() == want.tobytes(), (mode, _where(Wd, want))
        assert np.any(Wd[:2] != 0)
        if mode == IMPULSE:
            b.apply_impulses(drig["world"], drig["body"], Wd[:, 0:3], Wd[:, 3:6])
        else:
            _force_reference(b, drig, Wd)
        assert _everything(a) == _everything(b), mode
        for t in (a, b):
            _step(t, dsc, 2)
        assert _everything(a) == _everything(b), mode
    assert a.constraints(0).tobytes() == b.constraints(0).tobytes()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_that_need_the_handle_leave_the_rig_and_the_state_as_they_were(ctx):
    import mgf_amd
    import torch
    from mgf_amd import _capi
    INV = _capi.ERR_INVALID
    (a, b), scs = _twins(ctx, 2, seed=10)
    lens = _lengths(a)
    rig, u, planted = AC.main_rig(lens)
    a.set_actuators(rig)
    n, K = len(rig), a.n_worlds
    lib = mgf_amd.load_library()
    kept = _everything(a)
    nan, inf = np.nan, np.inf
    at = 11
    cases = [("world", -1), ("world", K), ("body", -1), ("body", lens[int(rig["world"][at])]), ("flags", 4), ("flags", 7), ("flags", 1 << 31),
             ("gain", nan), ("gain", inf), ("p", (0.0, nan, 0.0)), ("p", (inf, 0.0, 0.0)), ("d", (0.0, 0.0, -inf)), ("d", (nan, 0.0, 0.0)),
             ("lo", nan), ("hi", nan), ("lo", inf), ("hi", -inf)]
    for field, value in cases:
        bad = rig.copy()
        bad[field][at] = value
        if field in ("lo", "hi") and value in (inf, -inf):
            bad["lo" if field == "hi" else "hi"][at] = 0.0                   # lo > hi
        with pytest.raises(mgf_amd.MgfError) as e:
            a.set_actuators(bad)
        assert e.value.status == INV and "the rig was not changed" in str(e.value) and a.actuator_count() == n, (field, value, str(e.value))
    ok = rig.copy()
    ok["lo"][at], ok["hi"][at] = 0.25, 0.25                                   # lo == hi is a constant control
    a.set_actuators(ok)
    a.set_actuators(rig)
    # a control vector of another length than the rig, in either form, with or without somewhere to put the wrenches
    uu = np.ascontiguousarray(u)
    out = np.zeros((n, 6), np.float32)
    dev = torch.zeros(n + 6 * n + 8, dtype=torch.float32, device="cuda")
    _sync()
    up, wp = dev.data_ptr(), dev.data_ptr() + 4 * n
    for m in (n - 1, n + 1, 0):
        assert lib.mgf_batch_actuate(a._h, uu.ctypes.data, m, IMPULSE, out.ctypes.data) == INV and "actuator_count" in lib.mgf_last_error().decode()
        assert lib.mgf_batch_actuate_dev(a._h, up, m, FORCE, wp) == INV and "actuator_count" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_actuate(a._h, None, n, IMPULSE, None) == INV and "NULL" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_actuate_dev(a._h, None, n, IMPULSE, wp) == INV and "NULL" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_actuate(a._h, uu.ctypes.data, n, 2, None) == INV and "mode" in lib.mgf_last_error().decode()
    # the device form's own: an overlap of the two arrays (both are device memory: nothing here hands the call a host pointer)
    assert lib.mgf_batch_actuate_dev(a._h, up, n, IMPULSE, up + 4 * n - 4) == INV and "overlaps" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_actuate_dev(a._h, up + 24 * n - 4, n, IMPULSE, up) == INV and "overlaps" in lib.mgf_last_error().decode()
    _sync()
    assert not dev.any().item() and not out.any()                             # nothing was written
    assert a.actuator_count() == n and _everything(a) == kept == _everything(b)
    # the rig is as it was: the next call is the twin's apply_impulses, the next step the twin's
    W = a.actuate(u, IMPULSE, wrenches=True)
    want, _ = AC.rig_wrenches(rig, u, b.state(), lens)
    assert W.tobytes() == want.tobytes()
    b.apply_impulses(rig["world"], rig["body"], W[:, 0:3], W[:, 3:6])
    for t in (a, b):
        _step(t, scs)
    assert _everything(a) == _everything(b)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_kernel_uses_no_scratch_and_spills_nothing():
    from tests.util import kernel_resources
    rows = kernel_resources("k_batch_actuate")
    assert len(rows) == 4, sorted(rows)
    for name, v in rows.items():
        assert v[2] == "0" and v[4] == "0" and v[5] == "0", (name, v)
