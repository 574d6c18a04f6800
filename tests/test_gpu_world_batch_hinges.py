"""The hinges of a batch (mgf_batch_set_hinges / _set_hinge_targets / _set_hinge_targets_dev / _solve_hinges / _solve_hinges_dev;
WorldBatch.set_hinges / .set_hinge_targets / .set_hinge_targets_dev / .solve_hinges / .solve_hinges_dev) against their definition: v,
omega and the eight-float impulses equal the numpy restatement over state() and get() byte for byte (tests/batch_hinge_cases.py),
nothing else of state() and get() moves - on the worlds of the ball joints' tests: no hinge, one to the world, a chain in order and in
reverse, a star, two on one pair, a ring, and 256 shuffled hinges over 130 bodies, all interleaved in the caller's array, every flag
case dealt round them; iters 0, 1 and 4, beta 0 and 0.2, rows 0 and 2 of a table of three, both forms; the skips; the 257th hinge; the
refusals; bodies added; the table reset.  A rollout of a batch with hinges equals the defining loop
[apply_springs_dev] | actuate_dev | [solve_joints_dev] | solve_hinges_dev(row min(t, rows - 1)) | step(1) | gather_state | [traces]
by bytes - also when its ticks are undone and run again in mid-call.  And through the real tick a limited elbow stays in its range."""
import numpy as np
import pytest

from tests import batch_actuator_cases as AC
from tests import batch_hinge_cases as HC
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
    """a batch of HC.hinge_scenes(), ticked (delta leaves zero), then q, v and omega written into every body"""
    import mgf_amd
    scs = HC.hinge_scenes() if scs is None else scs
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    b.step(float(scs[0]["dt"]), scs[0]["iters"], HC.SETTLE_TICKS)
    q, v, om = HC.written_state(len(b))
    b.write_state(None, q=q, v=v, omega=om)
    return b


def _main_rig(b, beta=0.2):
    return HC.main_rig(_lengths(b), b.state(), beta=beta)


def _solve_dev(b, h, iters, row, impulses=True):
    """solve_hinges_dev between two waits for the whole device; the impulse buffer starts as 0x5A bytes: a row the call does not write shows"""
    import torch
    out = torch.full((b.hinge_count(), 8), FILL, dtype=torch.int32, device="cuda").view(torch.float32) if impulses else None
    _sync()
    b.solve_hinges_dev(h, iters, row, impulses_dev=out)
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
    import torch
    a, d = _batch(ctx), _batch(ctx)
    lens = _lengths(a)
    assert lens == list(HC.LENGTHS) and np.any(a.state()["delta"] != 0) and not GR._same(a, d)
    rig, planted, W = _main_rig(a, beta)
    assert a.hinge_count() == 0
    a.set_hinges(rig)
    d.set_hinges(rig)
    a.set_hinge_targets(W)                                                      # the host form of the table ...
    Wd = torch.from_numpy(W).cuda()
    d.set_hinge_targets_dev(Wd)                                                 # ... and the device form
    _sync()
    Wd.fill_(7.0)                                                               # (the table is the handle's copy)
    assert a.hinge_count() == len(rig) == 21 + HC.MAX and np.any(np.diff(rig["world"]) < 0) and W.shape == (HC.ROWS, len(rig))
    before, got_before = _full(a)
    want = HC.solve(rig, H, iters, W[0], before, lens)
    assert np.flatnonzero(want[3]).tolist() == planted and np.all(np.isfinite(want[0])) and np.all(np.isfinite(want[2]))
    P = a.solve_hinges(H, iters, 0, impulses=True)                              # the host form, row 0
    assert a.counter("drive_launches") == (1 if iters else 0) and mgf_amd.BATCH_HINGE_LAUNCHES == 1
    assert P.dtype == np.float32 and P.shape == (len(rig), 8)
    assert P.tobytes() == want[2].tobytes(), ("impulses", _where(P, want[2]))
    _check(a, before, got_before, want, "host form")
    Pd, launches = _solve_dev(d, H, iters, 0)                                   # the device form
    assert launches == (1 if iters else 0)
    if iters:
        assert Pd.tobytes() == want[2].tobytes(), ("impulses, device form", _where(Pd, want[2]))
    else:
        assert np.all(Pd.view(np.int32) == FILL)                                # iters == 0: nothing enqueued, nothing written
    _check(d, before, got_before, want, "device form")
    assert not GR._same(a, d)
    skipped = len(planted) if iters else 0
    assert a.counter("hinges_skipped") == skipped == d.counter("hinges_skipped") and not P[planted].any()
    if iters:
        moved = np.any(want[0] != before["v"], axis=1)
        off = np.concatenate([[0], np.cumsum(lens)])
        assert not moved[off[HC.BARE]:off[HC.BARE + 1]].any() and moved[off[HC.CHAIN]:off[HC.CHAIN] + 5].all()
        live = [i for i in range(len(rig)) if i not in planted]
        assert np.all(np.any(P[live, 0:3] != 0, axis=1)) and np.all(P[:, 7] == 0)
        case = np.arange(len(rig)) % 10
        assert np.any(P[case == 2, 5] > 0) and np.any(P[case == 3, 5] < 0) and np.any(P[case == 4, 5] < 0) and np.any(P[case == 6, 6] != 0)   # limits and motors acted
    # a second call, row 2 of the table, without the impulses: from the state the first left, no state kept between calls
    before2, got2 = _full(a)
    want2 = HC.solve(rig, H, iters, W[2], before2, lens)
    assert a.solve_hinges(H, iters, 2) is None
    none, launches = _solve_dev(d, H, iters, 2, impulses=False)
    assert none is None
    _check(a, before2, got2, want2, "host form, second call, row 2")
    _check(d, before2, got2, want2, "device form, second call, row 2")
    if iters:
        assert want2[1].tobytes() != HC.solve(rig, H, iters, W[0], before2, lens)[1].tobytes()     # the row matters
    assert a.counter("hinges_skipped") == 2 * skipped == d.counter("hinges_skipped")
    # the tick integrates what the hinges left: both forms stay twins
    sc = HC.hinge_scenes()[0]
    for t in (a, d):
        t.step(float(sc["dt"]), sc["iters"], 2)
    assert not GR._same(a, d)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_skipped_hinges_touch_nothing_and_are_counted(ctx):
    a = _batch(ctx)
    lens = _lengths(a)
    rig, planted, W = _main_rig(a, 0.0)
    rig["beta"][::2] = 0.2                                                      # h = 0: 0 / 0 where beta = 0, an infinite bias where not
    a.set_hinges(rig)
    a.set_hinge_targets(W)
    before, got_before = _full(a)
    want = HC.solve(rig, 0.0, 4, W[1], before, lens)
    assert want[3].all() and want[0].tobytes() == before["v"].tobytes()
    P = a.solve_hinges(0.0, 4, 1, impulses=True)
    assert not P.any() and a.counter("hinges_skipped") == len(rig) and a.counter("drive_launches") == 1
    _check(a, before, got_before, want, "h = 0")
    Pd, _ = _solve_dev(a, 0.0, 1, 1)
    assert not Pd.any() and a.counter("hinges_skipped") == 2 * len(rig)
    _check(a, before, got_before, want, "h = 0, device form")
    # the planted hinges alone are skipped at a usable h - the arm that overflows, the NaN target; the hinges around them are solved in their places
    want = HC.solve(rig, H, 4, W[1], before, lens)
    assert np.flatnonzero(want[3]).tolist() == planted and len(planted) == 2
    P = a.solve_hinges(H, 4, 1, impulses=True)
    assert P.tobytes() == want[2].tobytes() and a.counter("hinges_skipped") == 2 * len(rig) + 2
    _check(a, before, got_before, want, "the planted skips")
    # a NaN target is nothing to a hinge without MOTOR; a table row without the NaN solves the motor
    nan_at = [i for i in planted if rig["flags"][i] & HC.MOTOR][0]
    W2 = W.copy()
    W2[:, nan_at] = 0.5
    W2[:, np.flatnonzero((rig["flags"] & HC.MOTOR) == 0)[:5]] = np.nan
    a.set_hinge_targets(W2)
    before, got_before = _full(a)
    want = HC.solve(rig, H, 2, W2[0], before, lens)
    assert int(want[3].sum()) == 1
    P = a.solve_hinges(H, 2, 0, impulses=True)
    assert P.tobytes() == want[2].tobytes() and P[nan_at].any()
    _check(a, before, got_before, want, "NaN targets beside hinges without a motor")


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_rig_the_table_and_the_state_as_they_were_and_enqueue_nothing(ctx):
    import mgf_amd
    import torch
    from mgf_amd import _capi
    INV = _capi.ERR_INVALID
    a = _batch(ctx)
    lens = _lengths(a)
    rig, planted, W = _main_rig(a)
    a.set_hinges(rig)
    a.set_hinge_targets(W)
    n, K = len(rig), a.n_worlds
    lib = mgf_amd.load_library()
    kept = GR._everything(a)
    nan, inf = np.nan, np.inf
    at = int(np.flatnonzero((rig["other"] >= 0) & (rig["world"] == HC.FULL) & (rig["sh"] > 0.1))[3])
    nb = lens[HC.FULL]
    r0 = rig[at]
    tilted = (r0["ua"] + np.float32(0.05) * r0["ax"]) / np.float32(np.sqrt(1.0025))
    cases = [("world", -1, "world"), ("world", K, "world"), ("body", -1, "body"), ("body", nb, "body"), ("other", -2, "other"), ("other", nb, "other"),
             ("other", int(rig["body"][at]), "its body"), ("flags", 4, "flags"), ("flags", 1 << 31, "flags"), ("flags", 7, "flags"),
             ("pa", (0.0, nan, 0.0), "not finite"), ("pb", (inf, 0.0, 0.0), "not finite"), ("ax", (nan, 0.0, 0.0), "not finite"), ("ua", (0.0, 0.0, -inf), "not finite"),
             ("bx", (0.0, nan, 0.0), "not finite"), ("ub", (inf, 0.0, 0.0), "not finite"), ("beta", nan, "not finite"), ("beta", inf, "not finite"),
             ("tmax", nan, "not finite"), ("tmax", -inf, "not finite"), ("cm", nan, "not finite"), ("sm", inf, "not finite"), ("ch", -inf, "not finite"),
             ("sh", nan, "not finite"), ("beta", -0.1, "beta"), ("beta", 1.5, "beta"), ("tmax", -1.0, "tmax"),
             ("ax", r0["ax"] * np.float32(1.01), "unit length"), ("ua", r0["ua"] * np.float32(0.99), "unit length"), ("bx", r0["bx"] * np.float32(1.01), "unit length"),
             ("ub", (0.0, 0.0, 0.0), "unit length"), ("cm", 1.2, "unit length"), ("ch", 1.2, "unit length"),
             ("ua", tilted, "perpendicular"), ("ub", r0["bx"], "perpendicular"), ("sh", -r0["sh"], "sh is negative")]
    for field, value, word in cases:
        bad = rig.copy()
        bad[field][at] = value
        with pytest.raises(mgf_amd.MgfError) as e:
            a.set_hinges(bad)
        assert e.value.status == INV and "the rig was not changed" in str(e.value) and word in str(e.value) and a.hinge_count() == n, (field, value, str(e.value))
    # the order of the refusals: a record wrong in every way is refused for the first of them
    bad = rig.copy()
    bad["other"][at], bad["flags"][at], bad["pa"][at], bad["beta"][at], bad["tmax"][at] = bad["body"][at], 8, (nan, 0, 0), 2.0, -1.0
    bad["ax"][at], bad["ua"][at], bad["sh"][at] = r0["ax"] * np.float32(1.01), tilted, -r0["sh"]
    for fix, word in ((("other", r0["other"]), "its body"), (("flags", 3), "flags"), (("pa", r0["pa"]), "not finite"), (("beta", 1.0), "beta"), (("tmax", inf), "tmax"),
                      (("ax", r0["ax"]), "unit length"), (("ua", r0["ua"]), "perpendicular"), (("sh", r0["sh"]), "sh is negative")):
        with pytest.raises(mgf_amd.MgfError) as e:
            a.set_hinges(bad)
        assert word in str(e.value), (word, str(e.value))
        bad[fix[0]][at] = fix[1]
    # a 257th hinge on one world: refused behind every other check, the rig unchanged; on another world it is one more hinge
    more = np.concatenate([rig, HC.hinge(HC.FULL, 0, 1)])
    with pytest.raises(mgf_amd.MgfError) as e:
        a.set_hinges(more)
    assert e.value.status == INV and "256" in str(e.value) and "the rig was not changed" in str(e.value) and a.hinge_count() == n
    more["tmax"][5] = -1.0                                                     # (a record ahead of it that is wrong goes first)
    with pytest.raises(mgf_amd.MgfError) as e:
        a.set_hinges(more)
    assert "tmax" in str(e.value)
    # the table: rows, a NULL table, the device form's pointer - the table as it was
    dev = torch.zeros(3 * n + 8, dtype=torch.float32, device="cuda")
    for rows in (0, -1, (1 << 20) + 1):
        assert lib.mgf_batch_set_hinge_targets(a._h, W.ctypes.data, rows) == INV and "rows" in lib.mgf_last_error().decode()
        assert lib.mgf_batch_set_hinge_targets_dev(a._h, dev.data_ptr(), rows) == INV and "rows" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_set_hinge_targets(a._h, None, 3) == INV and "NULL" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_set_hinge_targets_dev(a._h, None, 3) == INV and "NULL" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_set_hinge_targets_dev(a._h, dev.data_ptr() + 2, 3) == INV and "aligned" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_set_hinge_targets_dev(a._h, W.ctypes.data, 3) == INV and "device memory" in lib.mgf_last_error().decode()
    # the solve calls: a time step that is not finite, negative iters, a row outside the table; the device form's pointer
    out = np.zeros((n, 8), np.float32)
    imp = torch.zeros(8 * n + 8, dtype=torch.float32, device="cuda")
    _sync()
    a.get(*_all(a))                                                             # (a call that launches: "drive_launches" is not 0)
    assert a.counter("drive_launches") > 0
    for bad_h in (nan, inf, -inf):
        assert lib.mgf_batch_solve_hinges(a._h, bad_h, 4, 0, out.ctypes.data) == INV and "h is not finite" in lib.mgf_last_error().decode()
        assert lib.mgf_batch_solve_hinges_dev(a._h, bad_h, -1, 9, imp.data_ptr()) == INV and "h is not finite" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_solve_hinges(a._h, float(H), -1, 9, out.ctypes.data) == INV and "iters is negative" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_solve_hinges_dev(a._h, float(H), -1, 0, imp.data_ptr()) == INV and "iters is negative" in lib.mgf_last_error().decode()
    for row in (-1, HC.ROWS, 1 << 40):
        assert lib.mgf_batch_solve_hinges(a._h, float(H), 4, row, out.ctypes.data) == INV and "row is outside" in lib.mgf_last_error().decode()
        assert lib.mgf_batch_solve_hinges_dev(a._h, float(H), 0, row, imp.data_ptr() + 2) == INV and "row is outside" in lib.mgf_last_error().decode()   # behind the joints' refusals, ahead of the pointer
    assert lib.mgf_batch_solve_hinges_dev(a._h, float(H), 4, 0, imp.data_ptr() + 2) == INV and "aligned" in lib.mgf_last_error().decode()
    assert a.counter("drive_launches") == 0                                     # behind a refused call
    _sync()
    assert not imp.any().item() and not out.any() and not dev.any().item()      # nothing was written
    assert a.hinge_count() == n and GR._everything(a) == kept
    assert a.counter("hinges_skipped") == 0
    # an empty rig: MGF_OK, nothing enqueued; its table keeps its rows
    b = _batch(ctx)
    assert b.solve_hinges(H, 4, impulses=True).shape == (0, 8) and b.counter("drive_launches") == 0
    b.set_hinges(rig)
    b.set_hinges(rig[:0])
    b.solve_hinges_dev(H, 4)
    assert b.hinge_count() == 0 and b.counter("drive_launches") == 0 and GR._everything(b) == kept
    b.set_hinge_targets(np.zeros((4, 0), np.float32))
    b.solve_hinges(H, 4, 3)
    with pytest.raises(mgf_amd.MgfError):
        b.solve_hinges(H, 4, 4)
    # the rig and the table are as they were: the next call is the restatement's, row 2
    before, got_before = _full(a)
    want = HC.solve(rig, H, 2, W[2], before, lens)
    P = a.solve_hinges(H, 2, 2, impulses=True)
    assert P.tobytes() == want[2].tobytes()
    _check(a, before, got_before, want, "behind the refusals")


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_set_hinges_resets_the_table_to_one_row_of_zeros(ctx):
    import mgf_amd
    a = _batch(ctx)
    lens = _lengths(a)
    rig, planted, W = _main_rig(a)
    a.set_hinges(rig)
    before, got_before = _full(a)
    zeros = np.zeros(len(rig), np.float32)
    want = HC.solve(rig, H, 2, zeros, before, lens)                             # never set: one row of zeros - every motor a brake, none skipped for its target
    assert np.flatnonzero(want[3]).tolist() == [i for i in planted if not rig["flags"][i] & HC.MOTOR]
    P = a.solve_hinges(H, 2, 0, impulses=True)
    assert P.tobytes() == want[2].tobytes()
    _check(a, before, got_before, want, "a table never set")
    with pytest.raises(mgf_amd.MgfError, match="row is outside"):
        a.solve_hinges(H, 2, 1)
    a.set_hinge_targets(W)
    a.solve_hinges(H, 1, 2)                                                     # three rows now
    a.set_hinges(rig)                                                           # ... and one again
    with pytest.raises(mgf_amd.MgfError, match="row is outside"):
        a.solve_hinges(H, 2, 1)
    before, got_before = _full(a)
    want = HC.solve(rig, H, 3, zeros, before, lens)
    P, launches = _solve_dev(a, H, 3, 0)
    assert launches == 1 and P.tobytes() == want[2].tobytes()
    _check(a, before, got_before, want, "the table behind set_hinges")
    a.set_hinge_targets(W[1])                                                   # one row given as a vector
    before, got_before = _full(a)
    want = HC.solve(rig, H, 1, W[1], before, lens)
    assert a.solve_hinges(H, 1, 0, impulses=True).tobytes() == want[2].tobytes()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_bodies_added_behind_set_hinges_and_set_hinges_behind_added_bodies(ctx):
    scs = HC.hinge_scenes()
    a = _batch(ctx, scs)
    lens = _lengths(a)
    rig, planted, W = _main_rig(a)
    a.set_hinges(rig)
    a.set_hinge_targets(W)
    _solve_dev(a, H, 1, 0)                                                      # (the rig is up)
    # bodies added to an earlier world: flat indices move under the rig, every hinge stays on its bodies, the table stays
    a.add_bodies(HC.BARE, *AC.late_bodies(scs[HC.BARE]))
    lens2 = _lengths(a)
    assert lens2[HC.BARE] == lens[HC.BARE] + AC.LATE_BODIES and a.hinge_count() == len(rig)
    before, got_before = _full(a)
    want = HC.solve(rig, H, 4, W[1], before, lens2)
    P, launches = _solve_dev(a, H, 4, 1)
    assert launches == 1 and P.tobytes() == want[2].tobytes(), _where(P, want[2])
    _check(a, before, got_before, want, "bodies added behind set_hinges")
    # ... and a rig set behind them may name the new bodies
    new = lens[HC.BARE]
    rig2 = np.concatenate([rig, HC.hinge(HC.BARE, new, 0, pa=(0.1, 0, 0), pb=(0, 0.2, 0), beta=0.1, lo=-0.2, hi=0.3, flags=HC.LIMIT),
                           HC.hinge(HC.BARE, new + 1, -1, pb=(0, 3, 0), ax=(0, 1, 0), bx=(0, 1, 0), beta=0.1, tmax=np.inf, flags=HC.MOTOR)])
    a.set_hinges(rig2)
    W2 = np.concatenate([W[0], np.float32([0.0, 1.25])])
    a.set_hinge_targets(W2)
    before, got_before = _full(a)
    want = HC.solve(rig2, H, 4, W2, before, lens2)
    P, launches = _solve_dev(a, H, 4, 0)
    assert P.tobytes() == want[2].tobytes() and np.all(np.any(P[-2:] != 0, axis=1)) and P[-1, 6] != 0
    _check(a, before, got_before, want, "set_hinges behind added bodies")


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def _late_twins(ctx, cons_per_body, rows, joints=False, springs=False, traces=False):
    (a, b), scs, rig, u, planted = GR._late_twins(ctx, 2, cons_per_body_of_first=cons_per_body)
    lens = _lengths(a)
    hinges, W6 = HC.late_hinges(lens, a.state())
    for t in (a, b):
        t.set_hinges(hinges)
        t.set_hinge_targets(W6[:rows])
        if joints:
            t.set_joints(JC.anchor_midpoints(JC.late_joints(lens, seed=431), a.state(), lens))
        if springs:
            t.set_springs(SP.late_springs(lens)[0])
        if traces:
            t.set_touches(XC.late_touch_rig())
            t.set_sensors(YC.late_sensor_rig())
    return a, b, scs, u, planted, hinges, W6[:rows]


def _rollout(a, U, dt, iters, mode, body, traces):
    """A's side: one call.  Returns (state traces as bytes by name, sensor rows, touch rows, stats bytes)"""
    if traces:
        return GS._observe(a, U, dt, iters, mode, body, touches="full")
    got, stats = GR._rollout(a, U, dt, iters, mode, body)
    return got, None, None, stats


def _loop(b, U, dt, iters, mode, body, traces, rows):
    """B's side: the defining loop, call by call - the hinges behind the ball joints, tick t from row min(t, rows - 1)"""
    ticks, m = len(U), len(body)
    out = GR._buffers(ticks, m)
    srows = GS._sensor_buffer(ticks, b.sensor_count()) if traces else None
    tb = GT._touch_buffer(ticks, b.touch_count()) if traces else None
    ud, bd = GR._dev(U), GR._dev(body, np.int32)
    _sync()
    stats = b""
    for t in range(ticks):
        if b.spring_count():
            b.apply_springs_dev(dt)
        b.actuate_dev(ud[t], mode)
        if b.joint_count():
            b.solve_joints_dev(dt, iters)
        b.solve_hinges_dev(dt, iters, min(t, rows - 1))
        stats += bytes(b.step(dt, iters, 1))
        b.gather_state(bd, n=m, **{k: out[k][t] for k in out})
        if traces:
            b.read_touches_dev(tb[t])
            b.cast_sensors_dev(srows[t], kinds=GS.ALL)
    _sync()
    return {k: out[k].cpu().numpy().tobytes() for k in out}, (GS._hit_rows(srows) if traces else None), (GT._rows(tb) if traces else None), stats


@pytest.mark.parametrize("variant", ["alone_rows6", "all_rows3", "traces_rows1", "rerun_rows6", "rerun_all_traces_rows3"])
def test_a_rollout_with_hinges_is_the_defining_loop_also_when_ticks_are_run_again(ctx, variant):
    """rerun: cons_per_body = 1 - A's worlds outgrow their share in the MIDDLE of the rollout, so A's ticks are undone and run again
    while B never retries: hinges solved twice on a world that is run again, or not at all, show - a gate on `done` alone solves them
    twice.  rows3: ticks 3..5 read row 2; rows1: the one row holds for the whole call; rows6: a row a tick"""
    import mgf_amd
    rerun, every, traces = variant.startswith("rerun"), "all" in variant, "traces" in variant
    rows = int(variant[-1])
    a, b, scs, u, planted, hinges, W = _late_twins(ctx, 1 if rerun else None, rows, joints=every, springs=every, traces=traces)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    T = RC.T
    assert T == 6 and W.shape == (rows, len(hinges)) and len(hinges) == 24
    U = RC.controls(u, planted, ticks=T)
    body, outside = RC.traced(len(a), count=30)
    mode = FORCE if every else IMPULSE
    got, srows, touches, got_stats = _rollout(a, U, dt, iters, mode, body, traces)
    launches = a.counter("rollout_launches")
    want, want_rows, want_touches, want_stats = _loop(b, U, dt, iters, mode, body, traces, rows)
    per_tick = (mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK + mgf_amd.BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK +
                ((mgf_amd.BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK + mgf_amd.BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK) if every else 0) +
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
        assert srows.tobytes() == want_rows.tobytes() and touches.tobytes() == want_touches.tobytes()
    assert not GR._same(a, b), GR._same(a, b)
    assert a.counter("hinges_skipped") == b.counter("hinges_skipped") == 0
    assert a.counter("actuators_skipped") == b.counter("actuators_skipped") == T * len(planted)
    # the hinges did something, and the table's rows did: a twin without the rig, and one whose table is row 0 alone, end elsewhere
    c = GR._late_twins(ctx, 1, cons_per_body_of_first=None)[0][0]
    lens = _lengths(c)
    if every:
        c.set_joints(JC.anchor_midpoints(JC.late_joints(lens, seed=431), c.state(), lens))
        c.set_springs(SP.late_springs(lens)[0])
    plain, _ = GR._rollout(c, U, dt, iters, mode, body)
    assert plain["v"] != got["v"]
    if rows > 1:
        e = GR._late_twins(ctx, 1, cons_per_body_of_first=None)[0][0]
        e.set_hinges(hinges)
        e.set_hinge_targets(W[:1])
        if every:
            e.set_joints(JC.anchor_midpoints(JC.late_joints(lens, seed=431), e.state(), lens))
            e.set_springs(SP.late_springs(lens)[0])
        held, _ = GR._rollout(e, U, dt, iters, mode, body)
        row = len(got["omega"]) // T
        assert held["omega"][:row] == got["omega"][:row] and held["omega"][row:] != got["omega"][row:]     # tick 0 reads row 0 either way
    print("largest axis misalignment after", T, "ticks: with the hinges", HC.misalignment(hinges, a.state(), _lengths(a)).max(), "without",
          HC.misalignment(hinges, c.state(), lens).max())


def test_the_launches_of_a_rollout_with_and_without_a_hinge_rig(ctx):
    import mgf_amd
    import torch
    scs = RC.late_contact_scenes()
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    a, b, c, e, f = (mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True) for _ in range(5))
    lens = _lengths(a)
    hinges, W6 = HC.late_hinges(lens, a.state())
    for t in (a, b):
        t.set_hinges(hinges)
        t.set_hinge_targets(W6[:2])
    # no controls and no traces, a hinge rig that is not empty: NOT mgf_batch_step, but the loop solve_hinges_dev | step(1)
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    st = a.rollout_dev(RC.T, dt, iters, body=none)
    assert a.counter("rollout_launches") == RC.T * (mgf_amd.BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK + 1)      # and the launch that moves `act`
    stats = b""
    for t in range(RC.T):
        b.solve_hinges_dev(dt, iters, min(t, 1))
        stats += bytes(b.step(dt, iters, 1))
    assert bytes(st) == stats and not GR._same(a, b)
    c.step(dt, iters, RC.T)
    assert GR._same(a, c)                                                       # it differs from step(T) ...
    a.step(dt, iters, 2)                                                        # ... which applies no hinge, with or without a rig
    for _ in range(2):
        b.step(dt, iters, 1)
    assert not GR._same(a, b)
    # the host form is the device form
    a.rollout(RC.T, dt, iters, trace=())
    b.rollout_dev(RC.T, dt, iters, body=none)
    assert not GR._same(a, b)
    # an empty hinge rig: the ball joints' rollout gives the same bytes and the same launches as on a batch that never had one
    joints = JC.anchor_midpoints(JC.late_joints(lens), e.state(), lens)
    body, _ = RC.traced(len(e), count=10)
    e.set_hinges(hinges)
    e.set_hinge_targets(W6)
    e.set_hinges(hinges[:0])                                                    # set and cleared: empty
    for t in (e, f):
        t.set_joints(joints)
    ge, se = GR._rollout(e, RC.T, dt, iters, IMPULSE, body, T=RC.T)
    gf, sf = GR._rollout(f, RC.T, dt, iters, IMPULSE, body, T=RC.T)
    assert ge == gf and se == sf and not GR._same(e, f) and e.hinge_count() == 0
    parent = f.counter("rollout_launches")
    assert e.counter("rollout_launches") == parent == RC.T * (1 + mgf_amd.BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK)
    e.set_hinges(hinges)
    GR._rollout(e, RC.T, dt, iters, IMPULSE, body, T=RC.T)
    assert e.counter("rollout_launches") == parent + RC.T and e.counter("capacity_retries") == 0


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_limited_elbow_stays_in_its_range_through_the_real_tick_and_leaves_it_without_the_limit(ctx):
    """A two-body arm pinned to the world, gravity as the scene's force rows, the elbow limited to [-0.5, 0.7]; 64 ticks of a rollout
    that traces q and omega; theta from the trace in float64.  A limit acts from the call after the angle passed it, so one tick's
    travel is the definition's own overshoot: theta must stay within the range widened by twice the largest |dot(wd, A)| * dt of that
    trace.  The same rollout with the LIMIT flag cleared must leave the range by more than ten times that margin.  The initial turn
    (HC.ARM_SPIN) was chosen so that the float64 restatement with a stand-in tick does both on the CPU - asserted here first."""
    import mgf_amd
    sc = HC.arm_scene()
    dt = float(sc["dt"])
    inside, out, margin = HC.arm_verdict(*HC.arm_sim(True), dt)
    free = HC.arm_verdict(*HC.arm_sim(False), dt)
    print("CPU: with the limit theta leaves the range by", out, "margin", margin, "; without by", free[1])
    assert inside and free[1] > 10 * margin
    results = []
    for limit in (True, False):
        b = mgf_amd.WorldBatch.from_scenes(ctx, [sc], own_terrain=True)
        b.set_velocities([0, 0], [0, 1], sc["v0"], sc["omega0"])
        rig = HC.arm_rig(b.state(), limit)
        b.set_hinges(rig)
        tr = b.rollout(HC.ARM_TICKS, dt, HC.ARM_ITERS, trace=("q", "omega"))
        assert b.counter("hinges_skipped") == 0
        theta, rate = HC.arm_trace_angles(rig, tr["q"], tr["omega"])
        results.append(HC.arm_verdict(theta, rate, dt) + (float(theta.min()), float(theta.max()), float(HC.gaps(rig, b.state(), [2]).max()),
                                                           float(HC.misalignment(rig, b.state(), [2]).max())))
    (inside, out, margin, lo, hi, gap, tilt), free = results
    print("GPU: with the limit theta in [%.4f, %.4f], leaves the range by %.4f, margin %.4f, anchor gap %.4f, misalignment %.2e; without the limit it leaves by %.4f"
          % (lo, hi, out, margin, gap, tilt, free[1]))
    assert inside, (out, margin)
    assert free[1] > 10 * margin, (free[1], margin)
    assert lo < HC.ARM_LIMIT[0] + 0.05                                          # the limit was reached: it is what held the elbow
