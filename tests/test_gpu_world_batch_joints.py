"""The ball joints of a batch (mgf_batch_set_joints / _solve_joints / _solve_joints_dev; WorldBatch.set_joints / .solve_joints /
.solve_joints_dev) against their definition: v, omega and the impulses equal the numpy restatement over state() and get() byte for byte
(tests/batch_joint_cases.py), nothing else of state() and get() moves - on the smallest set of worlds at which the kernel can go
wrong: no joint, one world anchor, a chain in order and in reverse, a star, a hinge of two joints, a ring, and 256 shuffled joints over
130 bodies, all interleaved in the caller's array; iters 0, 1 and 4, beta 0 and 0.2, both forms; the skips; the 257th joint; the
refusals; bodies added; bodies of several components.  A rollout of a batch with joints equals the defining loop
[apply_springs_dev] | actuate_dev | solve_joints_dev | step(1) | gather_state | [traces]  by bytes - also when its ticks are undone and
run again in mid-call."""
import numpy as np
import pytest

from tests import batch_actuator_cases as AC
from tests import batch_joint_cases as JC
from tests import batch_rollout_cases as RC
from tests import batch_scan_cases as YC
from tests import batch_spring_cases as SP
from tests import batch_trace_cases as XC
from tests import test_gpu_world_batch_rollout as GR
from tests import test_gpu_world_batch_scan as GS
from tests import test_gpu_world_batch_trace as GT

pytestmark = pytest.mark.gpu
IMPULSE, FORCE = AC.IMPULSE, AC.FORCE
H = np.float32(1.0 / 60.0)
FILL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    import mgf_amd
    c = mgf_amd.Context(0)
    yield c
    c.close()


_sync, _lengths, _all = GR._sync, GR._lengths, GR._all


def _full(b):
    """what the restatement reads, and everything else a caller can read of the bodies: state() and get() of every body"""
    st = dict(b.state())
    got = b.get(*_all(b))
    st["inv_mass"], st["inv_moment"] = got["inv_mass"], got["inv_moment"]
    return st, got


def _batch(ctx, scs=None):
    """a batch of JC.joint_scenes(), ticked twice (delta leaves zero), then q, v and omega written into every body"""
    import mgf_amd
    scs = JC.joint_scenes() if scs is None else scs
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    b.step(float(scs[0]["dt"]), scs[0]["iters"], JC.SETTLE_TICKS)
    q, v, om = JC.written_state(len(b))
    b.write_state(None, q=q, v=v, omega=om)
    return b


def _main_rig(b, beta=0.2):
    st = b.state()
    return JC.main_rig(_lengths(b), (st["x"] + st["delta"]).astype(np.float32), beta=beta)


def _solve_dev(b, h, iters, impulses=True):
    """solve_joints_dev between two waits for the whole device; the impulse buffer starts as 0x5A bytes: a row the call does not write shows"""
    import torch
    out = torch.full((b.joint_count(), 3), FILL, dtype=torch.int32, device="cuda").view(torch.float32) if impulses else None
    _sync()
    b.solve_joints_dev(h, iters, impulses_dev=out)
    launches = b.counter("drive_launches")
    _sync()
    return (out.cpu().numpy() if impulses else None), launches


def _where(got, want):
    return [i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()][:8]


def _check(b, before, got_before, want, what):
    """the batch after a call: v and omega the restatement's, everything else of state() and get() as it was"""
    st, got = _full(b)
    assert st["v"].tobytes() == want[0].tobytes(), (what, "v", _where(st["v"], want[0]))
    assert st["omega"].tobytes() == want[1].tobytes(), (what, "omega", _where(st["omega"], want[1]))
    for k in ("x", "q", "delta"):
        assert st[k].tobytes() == before[k].tobytes(), (what, k)
    assert got["linear"].tobytes() == want[0].tobytes() and got["angular"].tobytes() == want[1].tobytes(), what
    for k in ("x", "restitution", "friction", "inv_mass", "inv_moment", "force", "torque"):
        assert got[k].tobytes() == got_before[k].tobytes(), (what, k)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 0.2])
@pytest.mark.parametrize("iters", [0, 1, 4])
def test_a_call_is_the_restatement_by_bytes_through_both_forms(ctx, iters, beta):
    import mgf_amd
    a, d = _batch(ctx), _batch(ctx)
    lens = _lengths(a)
    assert lens == list(JC.LENGTHS) and np.any(a.state()["delta"] != 0) and not GR._same(a, d)
    rig, planted = _main_rig(a, beta)
    assert a.joint_count() == 0
    for t in (a, d):
        t.set_joints(rig)
    assert a.joint_count() == len(rig) == 21 + JC.MAX and np.any(np.diff(rig["world"]) < 0)
    before, got_before = _full(a)
    want = JC.solve(rig, H, iters, before, lens)
    assert np.flatnonzero(want[3]).tolist() == planted and np.all(np.isfinite(want[0])) and np.all(np.isfinite(want[2]))
    P = a.solve_joints(H, iters, impulses=True)                                 # the host form
    assert a.counter("drive_launches") == (1 if iters else 0) and mgf_amd.BATCH_JOINT_LAUNCHES == 1
    assert P.dtype == np.float32 and P.shape == (len(rig), 3)
    assert P.tobytes() == want[2].tobytes(), ("impulses", _where(P, want[2]))
    _check(a, before, got_before, want, "host form")
    Pd, launches = _solve_dev(d, H, iters)                                      # the device form
    assert launches == (1 if iters else 0)
    if iters:
        assert Pd.tobytes() == want[2].tobytes(), ("impulses, device form", _where(Pd, want[2]))
    else:
        assert np.all(Pd.view(np.int32) == FILL)                                # iters == 0: nothing enqueued, nothing written
    _check(d, before, got_before, want, "device form")
    assert not GR._same(a, d)
    skipped = len(planted) if iters else 0
    assert a.counter("joints_skipped") == skipped == d.counter("joints_skipped") and not P[planted].any()
    if iters:
        moved = np.any(want[0] != before["v"], axis=1)
        off = np.concatenate([[0], np.cumsum(lens)])
        assert not moved[off[JC.BARE]:off[JC.BARE + 1]].any() and moved[off[JC.CHAIN]:off[JC.CHAIN] + 5].all()
        assert np.all(np.any(P[[i for i in range(len(rig)) if i not in planted]] != 0, axis=1))
        # CHAIN and CHAIN_REV hold the same joints on the same state in the opposite order: the order matters, and both are the restatement's
        assert want[0][off[JC.CHAIN]:off[JC.CHAIN] + 5].tobytes() != want[0][off[JC.CHAIN_REV]:off[JC.CHAIN_REV] + 5].tobytes() or iters == 0
    # a second call, without the impulses: from the state the first left, no state kept between calls
    before2, got2 = _full(a)
    want2 = JC.solve(rig, H, iters, before2, lens)
    assert a.solve_joints(H, iters) is None
    none, launches = _solve_dev(d, H, iters, impulses=False)
    assert none is None
    _check(a, before2, got2, want2, "host form, second call")
    _check(d, before2, got2, want2, "device form, second call")
    assert a.counter("joints_skipped") == 2 * skipped == d.counter("joints_skipped")
    # the tick integrates what the joints left: both forms stay twins
    sc = JC.joint_scenes()[0]
    for t in (a, d):
        t.step(float(sc["dt"]), sc["iters"], 2)
    assert not GR._same(a, d)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_skipped_joints_touch_nothing_and_are_counted(ctx):
    a = _batch(ctx)
    lens = _lengths(a)
    rig, planted = _main_rig(a, 0.0)
    rig["beta"][::2] = 0.2                                                      # h = 0: 0 / 0 where beta = 0, an infinite bias where not
    a.set_joints(rig)
    before, got_before = _full(a)
    want = JC.solve(rig, 0.0, 4, before, lens)
    assert want[3].all() and want[0].tobytes() == before["v"].tobytes()
    P = a.solve_joints(0.0, 4, impulses=True)
    assert not P.any() and a.counter("joints_skipped") == len(rig) and a.counter("drive_launches") == 1
    _check(a, before, got_before, want, "h = 0")
    Pd, _ = _solve_dev(a, 0.0, 1)
    assert not Pd.any() and a.counter("joints_skipped") == 2 * len(rig)
    _check(a, before, got_before, want, "h = 0, device form")
    # the planted joint alone is skipped at a usable h; the joints around it on the same bodies are solved in their places
    want = JC.solve(rig, H, 4, before, lens)
    assert np.flatnonzero(want[3]).tolist() == planted
    P = a.solve_joints(H, 4, impulses=True)
    assert P.tobytes() == want[2].tobytes() and a.counter("joints_skipped") == 2 * len(rig) + 1
    _check(a, before, got_before, want, "the planted skip")


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_rig_and_the_state_as_they_were_and_enqueue_nothing(ctx):
    import mgf_amd
    import torch
    from mgf_amd import _capi
    INV = _capi.ERR_INVALID
    a = _batch(ctx)
    lens = _lengths(a)
    rig, planted = _main_rig(a)
    a.set_joints(rig)
    n, K = len(rig), a.n_worlds
    lib = mgf_amd.load_library()
    kept = GR._everything(a)
    nan, inf = np.nan, np.inf
    at = int(np.flatnonzero((rig["other"] >= 0) & (rig["world"] == JC.STAR))[2])
    nb = lens[JC.STAR]
    cases = [("world", -1, "world"), ("world", K, "world"), ("body", -1, "body"), ("body", nb, "body"), ("other", -2, "other"), ("other", nb, "other"),
             ("other", int(rig["body"][at]), "its body"), ("flags", 1, "flags"), ("flags", 1 << 31, "flags"), ("pad", 1.0, "pad"), ("pad", nan, "pad"),
             ("pa", (0.0, nan, 0.0), "not finite"), ("pb", (inf, 0.0, 0.0), "not finite"), ("beta", nan, "beta"), ("beta", -0.1, "beta"), ("beta", 1.5, "beta"),
             ("beta", inf, "beta")]
    for field, value, word in cases:
        bad = rig.copy()
        bad[field][at] = value
        with pytest.raises(mgf_amd.MgfError) as e:
            a.set_joints(bad)
        assert e.value.status == INV and "the rig was not changed" in str(e.value) and word in str(e.value) and a.joint_count() == n, (field, value, str(e.value))
    # the order of the refusals: a record wrong in every way is refused for the first of them
    bad = rig.copy()
    bad["other"][at], bad["flags"][at], bad["pa"][at], bad["beta"][at] = bad["body"][at], 1, (nan, 0, 0), 2.0
    for fix, word in ((("other", rig["other"][at]), "its body"), (("flags", 0), "flags"), (("pa", rig["pa"][at]), "not finite"), (("beta", 1.0), "beta")):
        with pytest.raises(mgf_amd.MgfError) as e:
            a.set_joints(bad)
        assert word in str(e.value), (word, str(e.value))
        bad[fix[0]][at] = fix[1]
    a.set_joints(bad)                                                           # beta = 1 and beta = 0 are allowed
    a.set_joints(rig)
    # a 257th joint on one world: refused, the rig unchanged; on another world it is one more joint
    more = np.concatenate([rig, JC.joint(JC.FULL, 0, 1)])
    with pytest.raises(mgf_amd.MgfError) as e:
        a.set_joints(more)
    assert e.value.status == INV and "256" in str(e.value) and "the rig was not changed" in str(e.value) and a.joint_count() == n
    more["world"][-1] = JC.BARE
    a.set_joints(more)
    assert a.joint_count() == n + 1
    a.set_joints(rig)
    # the solve calls: a time step that is not finite, negative iters; the device form's pointer
    out = np.zeros((n, 3), np.float32)
    dev = torch.zeros(3 * n + 8, dtype=torch.float32, device="cuda")
    _sync()
    a.get(*_all(a))                                                             # (a call that launches: "drive_launches" is not 0)
    assert a.counter("drive_launches") > 0
    for bad_h in (nan, inf, -inf):
        assert lib.mgf_batch_solve_joints(a._h, bad_h, 4, out.ctypes.data) == INV and "h is not finite" in lib.mgf_last_error().decode()
        assert lib.mgf_batch_solve_joints_dev(a._h, bad_h, 4, dev.data_ptr()) == INV and "h is not finite" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_solve_joints(a._h, float(H), -1, out.ctypes.data) == INV and "iters is negative" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_solve_joints_dev(a._h, float(H), -1, dev.data_ptr()) == INV and "iters is negative" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_solve_joints_dev(a._h, float(H), 4, dev.data_ptr() + 2) == INV and "aligned" in lib.mgf_last_error().decode()
    assert a.counter("drive_launches") == 0                                     # behind a refused call
    _sync()
    assert not dev.any().item() and not out.any()                               # nothing was written
    assert a.joint_count() == n and GR._everything(a) == kept
    assert a.counter("joints_skipped") == 0
    # an empty rig: MGF_OK, nothing enqueued
    b = _batch(ctx)
    assert b.solve_joints(H, 4, impulses=True).shape == (0, 3) and b.counter("drive_launches") == 0
    b.set_joints(rig)
    b.set_joints(rig[:0])
    b.solve_joints_dev(H, 4)
    assert b.joint_count() == 0 and b.counter("drive_launches") == 0 and GR._everything(b) == kept
    # the rig is as it was: the next call is the restatement's
    before, got_before = _full(a)
    want = JC.solve(rig, H, 2, before, lens)
    P = a.solve_joints(H, 2, impulses=True)
    assert P.tobytes() == want[2].tobytes()
    _check(a, before, got_before, want, "behind the refusals")


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_bodies_added_behind_set_joints_and_set_joints_behind_added_bodies(ctx):
    scs = JC.joint_scenes()
    a = _batch(ctx, scs)
    lens = _lengths(a)
    rig, planted = _main_rig(a)
    a.set_joints(rig)
    _solve_dev(a, H, 1)                                                         # (the rig is up)
    # bodies added to an earlier world: flat indices move under the rig, every joint stays on its bodies
    a.add_bodies(JC.BARE, *AC.late_bodies(scs[JC.BARE]))
    lens2 = _lengths(a)
    assert lens2[JC.BARE] == lens[JC.BARE] + AC.LATE_BODIES and a.joint_count() == len(rig)
    before, got_before = _full(a)
    want = JC.solve(rig, H, 4, before, lens2)
    P, launches = _solve_dev(a, H, 4)
    assert launches == 1 and P.tobytes() == want[2].tobytes(), _where(P, want[2])
    _check(a, before, got_before, want, "bodies added behind set_joints")
    # ... and a rig set behind them may name the new bodies
    new = lens[JC.BARE]
    rig2 = np.concatenate([rig, JC.joint(JC.BARE, new, 0, pa=(0.1, 0, 0), pb=(0, 0.2, 0), beta=0.1), JC.joint(JC.BARE, new + 1, -1, pb=(0, 3, 0), beta=0.1)])
    a.set_joints(rig2)
    before, got_before = _full(a)
    want = JC.solve(rig2, H, 4, before, lens2)
    P, launches = _solve_dev(a, H, 4)
    assert P.tobytes() == want[2].tobytes() and np.all(np.any(P[-2:] != 0, axis=1))
    _check(a, before, got_before, want, "set_joints behind added bodies")


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_with_bodies_of_several_components_is_answered(ctx):
    import mgf_amd
    from tests import batch_parts_cases as PC
    dsc = [PC.six_scenes()[PC.DUMBBELLS]]
    dt, iters = float(dsc[0]["dt"]), dsc[0]["iters"]
    a = mgf_amd.WorldBatch.from_scenes(ctx, dsc, own_terrain=True)
    a.step(dt, iters, 4)
    n = _lengths(a)[0]
    rig = np.concatenate([JC.joint(0, n - 1, 0, pa=(0.2, 0, 0), pb=(0, 0.3, 0), beta=0.2), JC.joint(0, n - 1, -1, pa=(0, 0.1, 0), pb=(0, 2, 0), beta=0.2),
                          JC.joint(0, 1, n - 2, pb=(0.1, 0.1, 0), beta=0.1)])     # dumbbells (the bodies of two parts come last)
    a.set_joints(rig)
    before, got_before = _full(a)
    want = JC.solve(rig, dt, 4, before, [n])
    P, launches = _solve_dev(a, dt, 4)
    assert launches == 1 and P.tobytes() == want[2].tobytes() and P.all()
    _check(a, before, got_before, want, "dumbbells")
    a.step(dt, iters, 2)
    assert a.counter("launches_per_tick") == 7 and a.counter("joints_skipped") == 0


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def _late_twins(ctx, cons_per_body, springs=False, traces=False):
    (a, b), scs, rig, u, planted = GR._late_twins(ctx, 2, cons_per_body_of_first=cons_per_body)
    lens = _lengths(a)
    joints = JC.anchor_midpoints(JC.late_joints(lens), a.state(), lens)
    for t in (a, b):
        t.set_joints(joints)
        if springs:
            t.set_springs(SP.late_springs(lens)[0])
        if traces:
            t.set_touches(XC.late_touch_rig())
            t.set_sensors(YC.late_sensor_rig())
    return a, b, scs, u, planted, joints


def _rollout(a, U, dt, iters, mode, body, traces):
    """A's side: one call.  Returns (state traces as bytes by name, sensor rows, touch rows, stats bytes)"""
    if traces:
        return GS._observe(a, U, dt, iters, mode, body, touches="full")
    got, stats = GR._rollout(a, U, dt, iters, mode, body)
    return got, None, None, stats


def _loop(b, U, dt, iters, mode, body, traces):
    """B's side: the defining loop, call by call, solve_joints_dev between actuate_dev and step(1)"""
    ticks, m = len(U), len(body)
    out = GR._buffers(ticks, m)
    rows = GS._sensor_buffer(ticks, b.sensor_count()) if traces else None
    tb = GT._touch_buffer(ticks, b.touch_count()) if traces else None
    ud, bd = GR._dev(U), GR._dev(body, np.int32)
    _sync()
    stats = b""
    for t in range(ticks):
        if b.spring_count():
            b.apply_springs_dev(dt)
        b.actuate_dev(ud[t], mode)
        b.solve_joints_dev(dt, iters)
        stats += bytes(b.step(dt, iters, 1))
        b.gather_state(bd, n=m, **{k: out[k][t] for k in out})
        if traces:
            b.read_touches_dev(tb[t])
            b.cast_sensors_dev(rows[t], kinds=GS.ALL)
    _sync()
    return {k: out[k].cpu().numpy().tobytes() for k in out}, (GS._hit_rows(rows) if traces else None), (GT._rows(tb) if traces else None), stats


@pytest.mark.parametrize("variant", ["plain", "springs", "traces", "rerun", "rerun_springs_traces"])
def test_a_rollout_with_joints_is_the_defining_loop_also_when_ticks_are_run_again(ctx, variant):
    """rerun: cons_per_body = 1 - A's worlds outgrow their share in the MIDDLE of the rollout, so A's ticks are undone and run again
    while B never retries: joints solved twice on a world that is run again, or not at all, show"""
    import mgf_amd
    rerun, springs, traces = variant.startswith("rerun"), "springs" in variant, "traces" in variant
    a, b, scs, u, planted, joints = _late_twins(ctx, 1 if rerun else None, springs, traces)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    T = XC.T if traces else RC.T
    U = RC.controls(u, planted, ticks=T)
    body, outside = RC.traced(len(a), count=30)
    mode = FORCE if springs else IMPULSE
    got, rows, touches, got_stats = _rollout(a, U, dt, iters, mode, body, traces)
    launches = a.counter("rollout_launches")
    want, want_rows, want_touches, want_stats = _loop(b, U, dt, iters, mode, body, traces)
    per_tick = (mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK + mgf_amd.BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK + (mgf_amd.BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK if springs else 0) +
                ((mgf_amd.BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK + mgf_amd.BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK) if traces else 0))
    if rerun:
        assert a.counter("capacity_retries") > 0 and b.counter("capacity_retries") == 0 and launches > T * per_tick
    else:
        assert a.counter("capacity_retries") == 0 and launches == T * per_tick
    for k, _ in GR.TRACES:
        row = len(got[k]) // T
        assert got[k] == want[k], (k, "ticks whose rows differ:", [t for t in range(T) if got[k][t * row:(t + 1) * row] != want[k][t * row:(t + 1) * row]])
    assert got_stats == want_stats
    if traces:
        assert rows.tobytes() == want_rows.tobytes() and touches.tobytes() == want_touches.tobytes()
    assert not GR._same(a, b), GR._same(a, b)
    assert a.counter("joints_skipped") == b.counter("joints_skipped") == 0
    assert a.counter("actuators_skipped") == b.counter("actuators_skipped") == T * len(planted)
    # the joints did something: a twin without the rig ends elsewhere, with its anchor points further apart - the joints take the
    # relative velocity of the anchor points out ahead of every tick, without them the lattice closes at its own rate
    c = GR._late_twins(ctx, 1, cons_per_body_of_first=None)[0][0]
    if springs:
        c.set_springs(SP.late_springs(_lengths(c))[0])
    plain, _ = GR._rollout(c, U, dt, iters, mode, body)
    assert plain["v"] != got["v"]
    held, free = JC.gaps(joints, a.state(), _lengths(a)), JC.gaps(joints, c.state(), _lengths(c))
    print("largest anchor gap after", T, "ticks: with the joints", held.max(), "without", free.max())
    assert held.max() < free.max()


def test_the_launches_of_a_rollout_with_and_without_a_joint_rig(ctx):
    import mgf_amd
    import torch
    scs = RC.late_contact_scenes()
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    a, b, c, e = (mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True) for _ in range(4))
    lens = _lengths(a)
    joints = JC.anchor_midpoints(JC.late_joints(lens), a.state(), lens)
    for t in (a, b):
        t.set_joints(joints)
    # no controls and no traces, a joint rig that is not empty: NOT mgf_batch_step, but the loop solve_joints_dev | step(1)
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    st = a.rollout_dev(RC.T, dt, iters, body=none)
    assert a.counter("rollout_launches") == RC.T * (mgf_amd.BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK + 1)      # and the launch that moves `act`
    stats = b""
    for _ in range(RC.T):
        b.solve_joints_dev(dt, iters)
        stats += bytes(b.step(dt, iters, 1))
    assert bytes(st) == stats and not GR._same(a, b)
    c.step(dt, iters, RC.T)
    assert GR._same(a, c)                                                       # it differs from step(T) ...
    a.step(dt, iters, 2)                                                        # ... which applies no joint, with or without a rig
    for _ in range(2):
        b.step(dt, iters, 1)
    assert not GR._same(a, b)
    # the host form is the device form
    a.rollout(RC.T, dt, iters, trace=())
    b.rollout_dev(RC.T, dt, iters, body=none)
    assert not GR._same(a, b)
    # an empty joint rig: launch for launch what it was - the parent's count; with the rig: the parent's count plus T
    e.rollout_dev(RC.T, dt, iters, body=none)
    assert e.counter("rollout_launches") == 0 and not GR._same(e, c)
    body, _ = RC.traced(len(e), count=10)
    e.set_joints(joints)
    e.set_joints(joints[:0])                                                    # set and cleared: empty
    GR._rollout(e, RC.T, dt, iters, IMPULSE, body, T=RC.T)
    parent = e.counter("rollout_launches")
    assert parent == RC.T and e.joint_count() == 0                              # the record launch alone
    e.set_joints(joints)
    GR._rollout(e, RC.T, dt, iters, IMPULSE, body, T=RC.T)
    assert e.counter("rollout_launches") == parent + RC.T and e.counter("capacity_retries") == 0
