"""The springs of a batch (mgf_batch_set_springs / _apply_springs / _apply_springs_dev; WorldBatch.set_springs / .apply_springs /
.apply_springs_dev) against their definition, on twin batches built from the same scenes with q, v and omega written in: the wrenches
equal the numpy restatement over state() bit for bit (tests/batch_spring_cases.py); the batch afterwards equals a twin that received
apply_impulses of the record list; worlds no spring names equal an untouched third twin; rigs of 1, 256, 257 and 600 springs; bodies
added behind set_springs; bodies of several components; the counters; the refusals.  A rollout of a batch with springs equals the
four-call loop  apply_springs_dev | actuate_dev | step(1) | gather_state  by bytes - also when its ticks are undone and run again in
mid-call - and two spheres on a damped spring come to rest one rest length apart."""
import numpy as np
import pytest

from tests import batch_actuator_cases as AC
from tests import batch_rollout_cases as RC
from tests import batch_spring_cases as SP

pytestmark = pytest.mark.gpu
IMPULSE, FORCE = AC.IMPULSE, AC.FORCE
TRACES = (("x", 3), ("q", 4), ("v", 3), ("omega", 3))
H = np.float32(1.0 / 60.0)


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


def _everything(b, worlds=None):
    """what a caller can read of the batch: state() and get() of every body (of the given worlds), the constraint lists - as bytes"""
    w, bd = _all(b)
    st = b.state()
    got = b.get(w, bd)
    keep = np.ones(len(w), bool) if worlds is None else np.isin(w, worlds)
    ks = range(b.n_worlds) if worlds is None else worlds
    return [st[k][keep].tobytes() for k in SP.STATE] + [got[keep].tobytes()] + [b.constraints(k).tobytes() for k in ks]


def _diff(a, b):
    ea, eb = _everything(a), _everything(b)
    return [i for i in range(len(ea)) if ea[i] != eb[i]]


def _where(got, want):
    return [i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()][:8]


def _twins(ctx, count):
    """`count` batches of SP.spring_scenes(), ticked twice (delta leaves zero), then q, v and omega written into every body"""
    import mgf_amd
    scs = SP.spring_scenes()
    out = []
    for _ in range(count):
        b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
        b.step(float(scs[0]["dt"]), scs[0]["iters"], SP.SETTLE_TICKS)
        q, v, om = SP.written_state(len(b))
        b.write_state(None, q=q, v=v, omega=om)
        out.append(b)
    assert _lengths(out[0]) == list(SP.LENGTHS) and np.any(out[0].state()["delta"] != 0)
    for b in out[1:]:
        assert not _diff(b, out[0])
    return out, scs


def _main_rig(b):
    st = b.state()
    return SP.main_rig(_lengths(b), (st["x"] + st["delta"]).astype(np.float32), st["v"])


def _apply_dev(b, h=H, wrenches=True):
    """apply_springs_dev between two waits for the whole device; the wrench buffer starts as 0x5A bytes: a row the call does not write shows"""
    import torch
    n = b.spring_count()
    out = torch.full((n, 12), 0x5A5A5A5A, dtype=torch.int32, device="cuda").view(torch.float32) if wrenches else None
    _sync()
    b.apply_springs_dev(h, wrenches_out=out)
    launches = b.counter("drive_launches")
    _sync()
    return (out.cpu().numpy() if wrenches else None), launches


def _impulses(b, rig, W):
    b.apply_impulses(*SP.records(rig, W))


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_call_is_apply_impulses_of_the_restated_record_list_through_both_forms(ctx):
    import mgf_amd
    (a, b, c, d), scs = _twins(ctx, 4)
    lens = _lengths(a)
    rig, planted = _main_rig(a)
    assert a.spring_count() == 0
    for t in (a, d):
        t.set_springs(rig)
    assert a.spring_count() == len(rig) and 190 <= len(rig) <= 230
    other_rigs = [a.actuator_count(), a.sensor_count(), a.zone_count(), a.touch_count(), a.feeler_count(), a.camera_count()]
    want, skipped = SP.rig_wrenches(rig, H, a.state(), lens)
    assert sorted(np.flatnonzero(skipped).tolist()) == sorted(planted)
    W = a.apply_springs(H, wrenches=True)                                       # the host form
    assert a.counter("drive_launches") == 2 == mgf_amd.BATCH_SPRING_LAUNCHES
    assert W.dtype == np.float32 and W.shape == (len(rig), 12)
    assert W.tobytes() == want.tobytes(), ("wrenches", _where(W, want))
    Wd, launches = _apply_dev(d)                                                # the device form
    assert launches <= mgf_amd.BATCH_SPRING_LAUNCHES and Wd.tobytes() == want.tobytes(), ("wrenches, device form", _where(Wd, want))
    assert np.all(W[planted] == 0) and a.counter("springs_skipped") == len(planted) == d.counter("springs_skipped")
    assert not W[rig["other"] < 0][:, 6:12].any() and np.any(W[rig["other"] >= 0][:, 6:12] != 0)
    _impulses(b, rig, want)
    assert not _diff(a, b), _diff(a, b)
    assert not _diff(d, b), _diff(d, b)
    assert _diff(a, c)
    bare = [SP.BARE_WORLD, SP.EMPTY_WORLD]
    assert _everything(a, bare) == _everything(c, bare)                         # worlds no spring names: the untouched twin's
    st_a, st_c = a.state(), c.state()
    for k in ("x", "q", "delta"):
        assert st_a[k].tobytes() == st_c[k].tobytes(), k                        # nothing but velocities is written
    w, bd = _all(a)
    ga, gc = a.get(w, bd), c.get(w, bd)
    for k in ("force", "torque", "x", "inv_mass", "inv_moment"):
        assert ga[k].tobytes() == gc[k].tobytes(), k
    assert [a.actuator_count(), a.sensor_count(), a.zone_count(), a.touch_count(), a.feeler_count(), a.camera_count()] == other_rigs == [0] * 6
    for t in (a, b, c, d):
        t.step(float(scs[0]["dt"]), scs[0]["iters"], 3)
    assert not _diff(a, b) and not _diff(d, b)
    assert _everything(a, bare) == _everything(c, bare)
    # without the wrenches the call does the same; the skips accumulate
    want2, skipped2 = SP.rig_wrenches(rig, H, a.state(), lens)
    assert int(skipped2.sum()) == 2                                             # (the body of the len == 0 spring has moved off its anchor)
    assert a.apply_springs(H) is None
    none, launches = _apply_dev(d, wrenches=False)
    assert none is None and launches == 2
    _impulses(b, rig, want2)
    assert not _diff(a, b) and not _diff(d, b)
    assert a.counter("springs_skipped") == len(planted) + 2 == d.counter("springs_skipped")
    assert a.counter("actuators_skipped") == 0 == a.counter("device_skipped")


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 256, 257, 600])
def test_rigs_of_every_size_and_bodies_added_behind_set_springs(ctx, count):
    import mgf_amd
    (a, b), scs = _twins(ctx, 2)
    lens = _lengths(a)
    rig = SP.sized_rig(lens, count)
    a.set_springs(rig)
    want, skipped = SP.rig_wrenches(rig, H, a.state(), lens)
    assert not skipped.any()
    W, launches = _apply_dev(a)
    assert launches <= mgf_amd.BATCH_SPRING_LAUNCHES and W.tobytes() == want.tobytes(), _where(W, want)
    _impulses(b, rig, want)
    assert not _diff(a, b), _diff(a, b)
    # bodies added to an earlier world: flat indices move under the rig, every spring stays on its bodies
    for t in (a, b):
        t.add_bodies(0, *AC.late_bodies(scs[0]))
    lens2 = _lengths(a)
    assert lens2[0] == lens[0] + AC.LATE_BODIES and a.spring_count() == count
    want, _ = SP.rig_wrenches(rig, H, a.state(), lens2)
    W, launches = _apply_dev(a)
    assert launches <= mgf_amd.BATCH_SPRING_LAUNCHES and W.tobytes() == want.tobytes(), _where(W, want)
    _impulses(b, rig, want)
    assert not _diff(a, b), _diff(a, b)
    assert a.counter("springs_skipped") == 0


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_with_bodies_of_several_components_is_answered(ctx):
    import mgf_amd
    from tests import batch_parts_cases as PC
    dsc = [PC.six_scenes()[PC.DUMBBELLS]]
    dt, iters = float(dsc[0]["dt"]), dsc[0]["iters"]
    a, b = (mgf_amd.WorldBatch.from_scenes(ctx, dsc, own_terrain=True) for _ in range(2))
    for t in (a, b):
        t.step(dt, iters, 4)
    n = _lengths(a)[0]
    rig = SP.sized_rig([n, n, n, n], 40)
    rig["world"] = 0
    rig["body"][:2], rig["other"][:2] = n - 1, [0, -1]                           # a dumbbell (the bodies of two parts come last), twice
    a.set_springs(rig)
    want, _ = SP.rig_wrenches(rig, dt, a.state(), [n])
    W, launches = _apply_dev(a, dt)
    assert launches == 2 and W.tobytes() == want.tobytes(), _where(W, want)
    assert np.any(W[:2] != 0)
    _impulses(b, rig, want)
    assert not _diff(a, b)
    for t in (a, b):
        t.step(dt, iters, 2)
    assert not _diff(a, b) and a.counter("launches_per_tick") == 7


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def _buffers(T, m, names=("x", "q", "v", "omega")):
    import torch
    return {k: torch.full((T, m, c), 0x5A5A5A5A, dtype=torch.int32, device="cuda").view(torch.float32) for k, c in TRACES if k in names}


def _dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _rollout(a, U, dt, iters, mode, body, T):
    """A's side: one rollout_dev; returns (traces as bytes by name, stats bytes)"""
    m = len(body)
    out = _buffers(T, m) if m else {}
    ud = _dev(U) if a.actuator_count() else T
    _sync()
    st = a.rollout_dev(ud, dt, iters, mode, body=_dev(body, np.int32), **out)
    _sync()
    return {k: out[k].cpu().numpy().tobytes() for k in out}, bytes(st)


def _loop(b, U, dt, iters, mode, body, T):
    """B's side: the defining loop of four calls"""
    m = len(body)
    out = _buffers(T, m) if m else {}
    ud = _dev(U) if b.actuator_count() else None
    bd = _dev(body, np.int32)
    _sync()
    stats = b""
    for t in range(T):
        b.apply_springs_dev(dt)
        if ud is not None:
            b.actuate_dev(ud[t], mode)
        stats += bytes(b.step(dt, iters, 1))
        if m:
            b.gather_state(bd, n=m, **{k: out[k][t] for k in out})
    _sync()
    return {k: out[k].cpu().numpy().tobytes() for k in out}, stats


def _late_twins(ctx, cons_per_body_of_first):
    import mgf_amd
    scs = RC.late_contact_scenes()
    out = []
    for i in range(2):
        b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
        if i == 0 and cons_per_body_of_first is not None:
            b.set_option("cons_per_body", cons_per_body_of_first)
        out.append(b)
    lens = _lengths(out[0])
    rig, u, planted = RC.late_rig(lens)
    springs, s_planted = SP.late_springs(lens)
    for b in out:
        b.set_actuators(rig)
        b.set_springs(springs)
    return out, scs, RC.controls(u, planted), planted, s_planted


@pytest.mark.parametrize("mode", [IMPULSE, FORCE])
@pytest.mark.parametrize("cons_per_body", [None, 1])
def test_a_rollout_with_springs_is_the_loop_of_four_calls_also_when_ticks_are_run_again(ctx, mode, cons_per_body):
    """cons_per_body = 1: A's worlds outgrow their share in the MIDDLE of the rollout, so A's ticks are undone and run again while B
    never retries - springs applied twice to a world that is run again (a gate on `done` alone), or not at all, show"""
    import mgf_amd
    (a, b), scs, U, planted, s_planted = _late_twins(ctx, cons_per_body)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    body, outside = RC.traced(len(a), count=30)
    got, got_stats = _rollout(a, U, dt, iters, mode, body, RC.T)
    launches = a.counter("rollout_launches")
    want, want_stats = _loop(b, U, dt, iters, mode, body, RC.T)
    per_tick = mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK + mgf_amd.BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK
    if cons_per_body is None:
        assert a.counter("capacity_retries") == 0 and launches == RC.T * per_tick == RC.T * (2 + 2)
    else:
        assert a.counter("capacity_retries") > 0 and b.counter("capacity_retries") == 0 and launches > RC.T * per_tick
    for k, _ in TRACES:
        row = len(got[k]) // RC.T
        assert got[k] == want[k], (k, "ticks whose rows differ:", [t for t in range(RC.T) if got[k][t * row:(t + 1) * row] != want[k][t * row:(t + 1) * row]])
    assert got_stats == want_stats
    assert not _diff(a, b), _diff(a, b)
    assert a.counter("springs_skipped") == b.counter("springs_skipped") == RC.T * len(s_planted)
    assert a.counter("actuators_skipped") == b.counter("actuators_skipped") == RC.T * len(planted)
    # the springs did something: a twin without them ends elsewhere
    rows = np.frombuffer(got["v"], np.float32).reshape(RC.T, len(body), 3)
    assert all(rows[t].tobytes() != rows[t + 1].tobytes() for t in range(RC.T - 1))


def test_a_rollout_without_controls_and_traces_is_the_stepping_call_of_a_batch_with_springs(ctx):
    import mgf_amd
    import torch
    scs = RC.late_contact_scenes()
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    a, b, c, e = (mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True) for _ in range(4))
    springs, s_planted = SP.late_springs(_lengths(a))
    for t in (a, b):
        t.set_springs(springs)
    none = np.zeros(0, np.int32)
    got, got_stats = _rollout(a, None, dt, iters, IMPULSE, none, RC.T)
    want, want_stats = _loop(b, None, dt, iters, IMPULSE, none, RC.T)
    assert got == want == {} and got_stats == want_stats and not _diff(a, b)
    assert a.counter("rollout_launches") == RC.T * (mgf_amd.BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK + 1)     # and the launch that moves `act`
    assert a.counter("springs_skipped") == b.counter("springs_skipped") == RC.T * len(s_planted)
    c.step(dt, iters, RC.T)
    assert _diff(a, c)                                                          # it differs from step(T) ...
    a.step(dt, iters, 2)                                                        # ... which applies no spring, with or without a rig
    b.step(dt, iters, 2)
    assert not _diff(a, b)
    # a batch whose spring rig is empty: launch for launch what it was
    st = e.rollout_dev(RC.T, dt, iters, body=torch.zeros(0, dtype=torch.int32, device="cuda"))
    assert len(st) == RC.T * e.n_worlds and e.counter("rollout_launches") == 0 and not _diff(e, c)
    body, _ = RC.traced(len(e), count=10)
    e.set_springs(springs)
    e.set_springs(springs[:0])                                                  # set and cleared: empty
    _rollout(e, None, dt, iters, IMPULSE, body, RC.T)
    assert e.counter("rollout_launches") == RC.T and e.spring_count() == 0      # the record launch alone
    rig, u, planted = RC.late_rig(_lengths(e))
    e.set_actuators(rig)
    _rollout(e, RC.controls(u, planted), dt, iters, IMPULSE, body, RC.T)
    assert e.counter("rollout_launches") == 2 * RC.T and e.counter("capacity_retries") == 0


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_two_spheres_on_a_damped_spring_come_to_rest_one_rest_length_apart(ctx):
    """relative motion r'' = -2 k (r - rest) - 2 c r' (unit masses): omega = sqrt(2 k) = 10 / s, and with c = 20 the slower root is
    -(20 - sqrt(300)) = -2.68 / s: after 5 s the offset of 1 has decayed below 2e-6.  The centre of mass moves only by the f32 rounding
    of equal and opposite impulses."""
    import mgf_amd
    sc = SP.free_pair()
    b = mgf_amd.WorldBatch.from_scenes(ctx, [sc], own_terrain=True)
    b.set_springs(SP.spring(0, 0, 1, rest=1.0, k=50.0, c=20.0))
    x0 = b.state()["x"] + b.state()["delta"]
    dt = 1.0 / 60.0
    xs = []
    for _ in range(3):
        xs.append(b.rollout(100, dt, sc["iters"], trace=("x",))["x"])
    x = np.concatenate(xs)
    assert x.shape == (300, 2, 3)
    length = np.linalg.norm(x[:, 1].astype(np.float64) - x[:, 0].astype(np.float64), axis=1)
    com = x.astype(np.float64).mean(axis=1)
    print("len after 1, 2, 3, 4, 5 s:", length[59::60].tolist(), "centre of mass moved by", float(np.abs(com - x0.astype(np.float64).mean(axis=0)).max()))
    assert abs(length[0] - 2.0) < 0.1 and np.all(np.diff(length[:60]) < 0)       # it closes from 2 ...
    assert abs(length[-1] - 1.0) < 1e-3                                         # ... to the rest length
    assert np.abs(com - x0.astype(np.float64).mean(axis=0)).max() < 1e-4
    assert b.counter("springs_skipped") == 0 and b.constraints(0).size == 0     # nothing touched anything


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_rig_and_the_state_as_they_were_and_enqueue_nothing(ctx):
    import mgf_amd
    import torch
    from mgf_amd import _capi
    INV = _capi.ERR_INVALID
    (a, b), scs = _twins(ctx, 2)
    lens = _lengths(a)
    rig, planted = _main_rig(a)
    a.set_springs(rig)
    n, K = len(rig), a.n_worlds
    lib = mgf_amd.load_library()
    kept = _everything(a)
    nan, inf = np.nan, np.inf
    at = int(np.flatnonzero(rig["other"] >= 0)[11])
    nb = lens[int(rig["world"][at])]
    cases = [("world", -1, "world"), ("world", K, "world"), ("body", -1, "body"), ("body", nb, "body"), ("other", -2, "other"), ("other", nb, "other"),
             ("other", int(rig["body"][at]), "its body"), ("flags", 1, "flags"), ("flags", 1 << 31, "flags"), ("pa", (0.0, nan, 0.0), "not finite"),
             ("pb", (inf, 0.0, 0.0), "not finite"), ("k", nan, "not finite"), ("k", inf, "not finite"), ("c", -inf, "not finite"), ("rest", nan, "not finite"),
             ("rest", -0.5, "negative"), ("lo", nan, "lo or hi"), ("hi", nan, "lo or hi"), ("lo", inf, "lo or hi"), ("hi", -inf, "lo or hi")]
    for field, value, word in cases:
        bad = rig.copy()
        bad[field][at] = value
        if field in ("lo", "hi") and value in (inf, -inf):
            bad["lo" if field == "hi" else "hi"][at] = 0.0                     # lo > hi
        with pytest.raises(mgf_amd.MgfError) as e:
            a.set_springs(bad)
        assert e.value.status == INV and "the rig was not changed" in str(e.value) and word in str(e.value) and a.spring_count() == n, (field, value, str(e.value))
    # the order of the refusals: a record wrong in every way is refused for the first of them
    bad = rig.copy()
    bad["other"][at], bad["flags"][at], bad["k"][at], bad["rest"][at], bad["lo"][at] = bad["body"][at], 1, nan, -1.0, nan
    for fix, word in ((("other", rig["other"][at]), "its body"), (("flags", 0), "flags"), (("k", 1.0), "not finite"), (("rest", 1.0), "negative"), (("lo", -1.0), "lo or hi")):
        with pytest.raises(mgf_amd.MgfError) as e:
            a.set_springs(bad)
        assert word in str(e.value), (word, str(e.value))
        bad[fix[0]][at] = fix[1]
    a.set_springs(bad)
    ok = rig.copy()
    ok["lo"][at], ok["hi"][at], ok["rest"][at] = 0.25, 0.25, 0.0               # lo == hi is a constant force; rest == 0 is allowed
    a.set_springs(ok)
    a.set_springs(rig)
    # the apply calls: a time step that is not finite; the device form's pointer
    out = np.zeros((n, 12), np.float32)
    dev = torch.zeros(12 * n + 8, dtype=torch.float32, device="cuda")
    _sync()
    a.get(*_all(a))                                                             # (a call that launches: "drive_launches" is not 0)
    assert a.counter("drive_launches") > 0
    for bad_h in (nan, inf, -inf):
        assert lib.mgf_batch_apply_springs(a._h, bad_h, out.ctypes.data) == INV and "h is not finite" in lib.mgf_last_error().decode()
        assert lib.mgf_batch_apply_springs_dev(a._h, bad_h, dev.data_ptr()) == INV and "h is not finite" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_apply_springs_dev(a._h, float(H), dev.data_ptr() + 2) == INV and "aligned" in lib.mgf_last_error().decode()
    assert a.counter("drive_launches") == 0                                     # behind a refused call
    # (the pointer is device memory throughout: nothing here hands the call a host pointer)
    _sync()
    assert not dev.any().item() and not out.any()                               # nothing was written
    assert a.spring_count() == n and _everything(a) == kept == _everything(b)
    # an empty rig: MGF_OK, nothing enqueued
    b.set_springs(rig[:0])
    assert b.apply_springs(H, wrenches=True).shape == (0, 12) and b.counter("drive_launches") == 0
    b.apply_springs_dev(H)
    assert b.counter("drive_launches") == 0 and _everything(b) == kept
    # the rig is as it was: the next call is the twin's apply_impulses
    W = a.apply_springs(H, wrenches=True)
    want, _ = SP.rig_wrenches(rig, H, b.state(), lens)
    assert W.tobytes() == want.tobytes()
    _impulses(b, rig, want)
    assert not _diff(a, b)
