"""The sliders of a batch (mgf_batch_set_sliders / _set_slider_targets / _set_slider_targets_dev / _solve_sliders / _solve_sliders_dev;
WorldBatch.set_sliders / .set_slider_targets / .set_slider_targets_dev / .solve_sliders / .solve_sliders_dev) against their definition:
v, omega and the eight-float impulses equal the numpy restatement over state() and get() byte for byte (tests/batch_slider_cases.py),
nothing else of state() and get() moves - on the worlds of the ball joints' tests: no slider, one to the world, a chain in order and in
reverse, a star, two on one pair, a ring, and 256 shuffled sliders over 130 bodies, all interleaved in the caller's array, every flag
case dealt round them; iters 0, 1 and 4, beta 0 and 0.2, rows 0 and 2 of a table of three, both forms; the skips; the 257th slider; the
refusals; bodies added; the table reset.  A rollout of a batch with sliders equals the defining loop
[apply_springs_dev] | actuate_dev | [solve_joints_dev] | [solve_hinges_dev] | solve_sliders_dev(row min(t, rows - 1)) | step(1) |
gather_state | [traces] by bytes - also when its ticks are undone and run again in mid-call.  And through the real tick a limited lift
stays in its range and a welded body keeps its pose."""
import numpy as np
import pytest

from tests import batch_actuator_cases as AC
from tests import batch_hinge_cases as HC
from tests import batch_joint_cases as JC
from tests import batch_rollout_cases as RC
from tests import batch_scan_cases as YC
from tests import batch_slider_cases as LC
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
    """a batch of LC.slider_scenes(), ticked (delta leaves zero), then q, v and omega written into every body"""
    import mgf_amd
    scs = LC.slider_scenes() if scs is None else scs
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    b.step(float(scs[0]["dt"]), scs[0]["iters"], LC.SETTLE_TICKS)
    q, v, om = LC.written_state(len(b))
    b.write_state(None, q=q, v=v, omega=om)
    return b


def _main_rig(b, beta=0.2):
    return LC.main_rig(_lengths(b), b.state(), beta=beta)


def _solve_dev(b, h, iters, row, impulses=True):
    """solve_sliders_dev between two waits for the whole device; the impulse buffer starts as 0x5A bytes: a row the call does not write shows"""
    import torch
    out = torch.full((b.slider_count(), 8), FILL, dtype=torch.int32, device="cuda").view(torch.float32) if impulses else None
    _sync()
    b.solve_sliders_dev(h, iters, row, impulses_dev=out)
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
    assert lens == list(LC.LENGTHS) and np.any(a.state()["delta"] != 0) and not GR._same(a, d)
    rig, planted, W = _main_rig(a, beta)
    assert a.slider_count() == 0
    a.set_sliders(rig)
    d.set_sliders(rig)
    a.set_slider_targets(W)                                                     # the host form of the table ...
    Wd = torch.from_numpy(W).cuda()
    d.set_slider_targets_dev(Wd)                                                # ... and the device form
    _sync()
    Wd.fill_(7.0)                                                               # (the table is the handle's copy)
    assert a.slider_count() == len(rig) == 21 + LC.MAX and np.any(np.diff(rig["world"]) < 0) and W.shape == (LC.ROWS, len(rig))
    before, got_before = _full(a)
    want = LC.solve(rig, H, iters, W[0], before, lens)
    assert np.flatnonzero(want[3]).tolist() == planted and np.all(np.isfinite(want[0])) and np.all(np.isfinite(want[2]))
    P = a.solve_sliders(H, iters, 0, impulses=True)                             # the host form, row 0
    assert a.counter("drive_launches") == (1 if iters else 0) and mgf_amd.BATCH_SLIDER_LAUNCHES == 1
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
    assert a.counter("sliders_skipped") == skipped == d.counter("sliders_skipped") and not P[planted].any()
    if iters:
        moved = np.any(want[0] != before["v"], axis=1)
        off = np.concatenate([[0], np.cumsum(lens)])
        assert not moved[off[LC.BARE]:off[LC.BARE + 1]].any() and moved[off[LC.CHAIN]:off[LC.CHAIN] + 5].all()
        live = [i for i in range(len(rig)) if i not in planted]
        assert np.all(np.any(P[live, 4:7] != 0, axis=1)) and np.all(P[:, 7] == 0)
        case = np.arange(len(rig)) % 10
        if beta:                                                                # (beta = 0: lb = 0, a limit only stops what moves against it)
            assert np.any(P[case == 2, 2] > 0) and np.any(P[case == 3, 2] < 0)
        assert np.any(P[case == 9, 2] != 0) and np.any(P[case == 5, 3] != 0)    # locks and motors acted
    # a second call, row 2 of the table, without the impulses: from the state the first left, no state kept between calls
    before2, got2 = _full(a)
    want2 = LC.solve(rig, H, iters, W[2], before2, lens)
    assert a.solve_sliders(H, iters, 2) is None
    none, launches = _solve_dev(d, H, iters, 2, impulses=False)
    assert none is None
    _check(a, before2, got2, want2, "host form, second call, row 2")
    _check(d, before2, got2, want2, "device form, second call, row 2")
    if iters:
        assert want2[1].tobytes() != LC.solve(rig, H, iters, W[0], before2, lens)[1].tobytes()     # the row matters
    assert a.counter("sliders_skipped") == 2 * skipped == d.counter("sliders_skipped")
    # the tick integrates what the sliders left: both forms stay twins
    sc = LC.slider_scenes()[0]
    for t in (a, d):
        t.step(float(sc["dt"]), sc["iters"], 2)
    assert not GR._same(a, d)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_skipped_sliders_touch_nothing_and_are_counted(ctx):
    a = _batch(ctx)
    lens = _lengths(a)
    rig, planted, W = _main_rig(a, 0.0)
    rig["beta"][::2] = 0.2                                                      # h = 0: 0 / 0 where beta = 0, infinite biases where not
    a.set_sliders(rig)
    a.set_slider_targets(W)
    before, got_before = _full(a)
    want = LC.solve(rig, 0.0, 4, W[1], before, lens)
    assert want[3].all() and want[0].tobytes() == before["v"].tobytes()
    P = a.solve_sliders(0.0, 4, 1, impulses=True)
    assert not P.any() and a.counter("sliders_skipped") == len(rig) and a.counter("drive_launches") == 1
    _check(a, before, got_before, want, "h = 0")
    Pd, _ = _solve_dev(a, 0.0, 1, 1)
    assert not Pd.any() and a.counter("sliders_skipped") == 2 * len(rig)
    _check(a, before, got_before, want, "h = 0, device form")
    # the planted sliders alone are skipped at a usable h - the arm that overflows, the NaN target; the sliders around them are solved in their places
    want = LC.solve(rig, H, 4, W[1], before, lens)
    assert np.flatnonzero(want[3]).tolist() == planted and len(planted) == 2
    P = a.solve_sliders(H, 4, 1, impulses=True)
    assert P.tobytes() == want[2].tobytes() and a.counter("sliders_skipped") == 2 * len(rig) + 2
    _check(a, before, got_before, want, "the planted skips")
    # a NaN target is nothing to a slider without MOTOR; a table row without the NaN solves the motor
    nan_at = [i for i in planted if rig["flags"][i] & LC.MOTOR][0]
    W2 = W.copy()
    W2[:, nan_at] = 0.5
    W2[:, np.flatnonzero((rig["flags"] & LC.MOTOR) == 0)[:5]] = np.nan
    a.set_slider_targets(W2)
    before, got_before = _full(a)
    want = LC.solve(rig, H, 2, W2[0], before, lens)
    assert int(want[3].sum()) == 1
    P = a.solve_sliders(H, 2, 0, impulses=True)
    assert P.tobytes() == want[2].tobytes() and P[nan_at].any()
    _check(a, before, got_before, want, "NaN targets beside sliders without a motor")


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_rig_the_table_and_the_state_as_they_were_and_enqueue_nothing(ctx):
    import mgf_amd
    import torch
    from mgf_amd import _capi
    INV = _capi.ERR_INVALID
    a = _batch(ctx)
    lens = _lengths(a)
    rig, planted, W = _main_rig(a)
    a.set_sliders(rig)
    a.set_slider_targets(W)
    n, K = len(rig), a.n_worlds
    lib = mgf_amd.load_library()
    kept = GR._everything(a)
    nan, inf = np.nan, np.inf
    at = int(np.flatnonzero((rig["other"] >= 0) & (rig["world"] == LC.FULL) & (rig["flags"] == LC.LIMIT))[3])
    assert at not in planted
    nb = lens[LC.FULL]
    r0 = rig[at]
    tilted = (r0["ua"] + np.float32(0.05) * r0["ax"]) / np.float32(np.sqrt(1.0025))
    cases = [("world", -1, "world"), ("world", K, "world"), ("body", -1, "body"), ("body", nb, "body"), ("other", -2, "other"), ("other", nb, "other"),
             ("other", int(rig["body"][at]), "its body"), ("flags", 8, "flags"), ("flags", 1 << 31, "flags"), ("flags", 16 | 1, "flags"),
             ("flags", 5, "MGF_SLIDER_LOCK stands beside"), ("flags", 6, "MGF_SLIDER_LOCK stands beside"), ("flags", 7, "MGF_SLIDER_LOCK stands beside"),
             ("pa", (0.0, nan, 0.0), "not finite"), ("pb", (inf, 0.0, 0.0), "not finite"), ("ax", (nan, 0.0, 0.0), "not finite"), ("ua", (0.0, 0.0, -inf), "not finite"),
             ("bx", (0.0, nan, 0.0), "not finite"), ("ub", (inf, 0.0, 0.0), "not finite"), ("beta", nan, "not finite"), ("beta", inf, "not finite"),
             ("fmax", nan, "not finite"), ("fmax", -inf, "not finite"), ("lo", nan, "not finite"), ("lo", -inf, "not finite"), ("hi", inf, "not finite"),
             ("pad0", nan, "not finite"), ("pad1", inf, "not finite"), ("pad0", 1.0, "pad0 or pad1"), ("pad1", -2.0, "pad0 or pad1"),
             ("beta", -0.1, "beta"), ("beta", 1.5, "beta"), ("fmax", -1.0, "fmax"), ("lo", float(r0["hi"]) + 0.5, "lo is above its hi"),
             ("ax", r0["ax"] * np.float32(1.01), "unit length"), ("ua", r0["ua"] * np.float32(0.99), "unit length"), ("bx", r0["bx"] * np.float32(1.01), "unit length"),
             ("ub", (0.0, 0.0, 0.0), "unit length"), ("ua", tilted, "perpendicular"), ("ub", r0["bx"], "perpendicular")]
    for field, value, word in cases:
        bad = rig.copy()
        bad[field][at] = value
        with pytest.raises(mgf_amd.MgfError) as e:
            a.set_sliders(bad)
        assert e.value.status == INV and "the rig was not changed" in str(e.value) and word in str(e.value) and a.slider_count() == n, (field, value, str(e.value))
    # the order of the refusals: a record wrong in every way is refused for the first of them
    bad = rig.copy()
    bad["other"][at], bad["flags"][at], bad["pa"][at], bad["pad1"][at], bad["beta"][at], bad["fmax"][at] = bad["body"][at], 8 | 5, (nan, 0, 0), 3.0, 2.0, -1.0
    bad["lo"][at], bad["ax"][at], bad["ua"][at] = r0["hi"] + np.float32(1.0), r0["ax"] * np.float32(1.01), tilted
    for fix, word in ((("other", r0["other"]), "its body"), (("flags", 5), "flags hold a bit"), (("flags", 1), "MGF_SLIDER_LOCK stands beside"), (("pa", r0["pa"]), "not finite"),
                      (("pad1", 0.0), "pad0 or pad1"), (("beta", 1.0), "beta"), (("fmax", inf), "fmax"), (("lo", r0["lo"]), "lo is above its hi"),
                      (("ax", r0["ax"]), "unit length"), (("ua", r0["ua"]), "perpendicular")):
        with pytest.raises(mgf_amd.MgfError) as e:
            a.set_sliders(bad)
        assert word in str(e.value), (word, str(e.value))
        bad[fix[0]][at] = fix[1]
    # a 257th slider on one world: refused behind every other check, the rig unchanged; on another world it is one more slider
    more = np.concatenate([rig, LC.slider(LC.FULL, 0, 1)])
    with pytest.raises(mgf_amd.MgfError) as e:
        a.set_sliders(more)
    assert e.value.status == INV and "256" in str(e.value) and "the rig was not changed" in str(e.value) and a.slider_count() == n
    more["fmax"][5] = -1.0                                                     # (a record ahead of it that is wrong goes first)
    with pytest.raises(mgf_amd.MgfError) as e:
        a.set_sliders(more)
    assert "fmax" in str(e.value)
    # the table: rows, a NULL table, the device form's pointer - the table as it was
    dev = torch.zeros(3 * n + 8, dtype=torch.float32, device="cuda")
    for rows in (0, -1, (1 << 20) + 1):
        assert lib.mgf_batch_set_slider_targets(a._h, W.ctypes.data, rows) == INV and "rows" in lib.mgf_last_error().decode()
        assert lib.mgf_batch_set_slider_targets_dev(a._h, dev.data_ptr(), rows) == INV and "rows" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_set_slider_targets(a._h, None, 3) == INV and "NULL" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_set_slider_targets_dev(a._h, None, 3) == INV and "NULL" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_set_slider_targets_dev(a._h, dev.data_ptr() + 2, 3) == INV and "aligned" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_set_slider_targets_dev(a._h, W.ctypes.data, 3) == INV and "device memory" in lib.mgf_last_error().decode()
    # the solve calls: a time step that is not finite, negative iters, a row outside the table; the device form's pointer
    out = np.zeros((n, 8), np.float32)
    imp = torch.zeros(8 * n + 8, dtype=torch.float32, device="cuda")
    _sync()
    a.get(*_all(a))                                                             # (a call that launches: "drive_launches" is not 0)
    assert a.counter("drive_launches") > 0
    for bad_h in (nan, inf, -inf):
        assert lib.mgf_batch_solve_sliders(a._h, bad_h, 4, 0, out.ctypes.data) == INV and "h is not finite" in lib.mgf_last_error().decode()
        assert lib.mgf_batch_solve_sliders_dev(a._h, bad_h, -1, 9, imp.data_ptr()) == INV and "h is not finite" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_solve_sliders(a._h, float(H), -1, 9, out.ctypes.data) == INV and "iters is negative" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_solve_sliders_dev(a._h, float(H), -1, 0, imp.data_ptr()) == INV and "iters is negative" in lib.mgf_last_error().decode()
    for row in (-1, LC.ROWS, 1 << 40):
        assert lib.mgf_batch_solve_sliders(a._h, float(H), 4, row, out.ctypes.data) == INV and "row is outside" in lib.mgf_last_error().decode()
        assert lib.mgf_batch_solve_sliders_dev(a._h, float(H), 0, row, imp.data_ptr() + 2) == INV and "row is outside" in lib.mgf_last_error().decode()   # behind the joints' refusals, ahead of the pointer
    assert lib.mgf_batch_solve_sliders_dev(a._h, float(H), 4, 0, imp.data_ptr() + 2) == INV and "aligned" in lib.mgf_last_error().decode()
    assert a.counter("drive_launches") == 0                                     # behind a refused call
    _sync()
    assert not imp.any().item() and not out.any() and not dev.any().item()      # nothing was written
    assert a.slider_count() == n and GR._everything(a) == kept
    assert a.counter("sliders_skipped") == 0
    # an empty rig: MGF_OK, nothing enqueued; its table keeps its rows
    b = _batch(ctx)
    assert b.solve_sliders(H, 4, impulses=True).shape == (0, 8) and b.counter("drive_launches") == 0
    b.set_sliders(rig)
    b.set_sliders(rig[:0])
    b.solve_sliders_dev(H, 4)
    assert b.slider_count() == 0 and b.counter("drive_launches") == 0 and GR._everything(b) == kept
    b.set_slider_targets(np.zeros((4, 0), np.float32))
    b.solve_sliders(H, 4, 3)
    with pytest.raises(mgf_amd.MgfError):
        b.solve_sliders(H, 4, 4)
    # the rig and the table are as they were: the next call is the restatement's, row 2
    before, got_before = _full(a)
    want = LC.solve(rig, H, 2, W[2], before, lens)
    P = a.solve_sliders(H, 2, 2, impulses=True)
    assert P.tobytes() == want[2].tobytes()
    _check(a, before, got_before, want, "behind the refusals")


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_set_sliders_resets_the_table_to_one_row_of_zeros(ctx):
    import mgf_amd
    a = _batch(ctx)
    lens = _lengths(a)
    rig, planted, W = _main_rig(a)
    a.set_sliders(rig)
    before, got_before = _full(a)
    zeros = np.zeros(len(rig), np.float32)
    want = LC.solve(rig, H, 2, zeros, before, lens)                             # never set: one row of zeros - every motor a brake, none skipped for its target
    assert np.flatnonzero(want[3]).tolist() == [i for i in planted if not rig["flags"][i] & LC.MOTOR]
    P = a.solve_sliders(H, 2, 0, impulses=True)
    assert P.tobytes() == want[2].tobytes()
    _check(a, before, got_before, want, "a table never set")
    with pytest.raises(mgf_amd.MgfError, match="row is outside"):
        a.solve_sliders(H, 2, 1)
    a.set_slider_targets(W)
    a.solve_sliders(H, 1, 2)                                                    # three rows now
    a.set_sliders(rig)                                                          # ... and one again
    with pytest.raises(mgf_amd.MgfError, match="row is outside"):
        a.solve_sliders(H, 2, 1)
    before, got_before = _full(a)
    want = LC.solve(rig, H, 3, zeros, before, lens)
    P, launches = _solve_dev(a, H, 3, 0)
    assert launches == 1 and P.tobytes() == want[2].tobytes()
    _check(a, before, got_before, want, "the table behind set_sliders")
    a.set_slider_targets(W[1])                                                  # one row given as a vector
    before, got_before = _full(a)
    want = LC.solve(rig, H, 1, W[1], before, lens)
    assert a.solve_sliders(H, 1, 0, impulses=True).tobytes() == want[2].tobytes()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_bodies_added_behind_set_sliders_and_set_sliders_behind_added_bodies(ctx):
    scs = LC.slider_scenes()
    a = _batch(ctx, scs)
    lens = _lengths(a)
    rig, planted, W = _main_rig(a)
    a.set_sliders(rig)
    a.set_slider_targets(W)
    _solve_dev(a, H, 1, 0)                                                      # (the rig is up)
    # bodies added to an earlier world: flat indices move under the rig, every slider stays on its bodies, the table stays
    a.add_bodies(LC.BARE, *AC.late_bodies(scs[LC.BARE]))
    lens2 = _lengths(a)
    assert lens2[LC.BARE] == lens[LC.BARE] + AC.LATE_BODIES and a.slider_count() == len(rig)
    before, got_before = _full(a)
    want = LC.solve(rig, H, 4, W[1], before, lens2)
    P, launches = _solve_dev(a, H, 4, 1)
    assert launches == 1 and P.tobytes() == want[2].tobytes(), _where(P, want[2])
    _check(a, before, got_before, want, "bodies added behind set_sliders")
    # ... and a rig set behind them may name the new bodies
    new = lens[LC.BARE]
    rig2 = np.concatenate([rig, LC.slider(LC.BARE, new, 0, pa=(0.1, 0, 0), pb=(0, 0.2, 0), beta=0.1, lo=-0.2, hi=0.3, flags=LC.LIMIT),
                           LC.slider(LC.BARE, new + 1, -1, pb=(0, 3, 0), ax=(0, 1, 0), bx=(0, 1, 0), beta=0.1, fmax=np.inf, flags=LC.MOTOR)])
    a.set_sliders(rig2)
    W2 = np.concatenate([W[0], np.float32([0.0, 1.25])])
    a.set_slider_targets(W2)
    before, got_before = _full(a)
    want = LC.solve(rig2, H, 4, W2, before, lens2)
    P, launches = _solve_dev(a, H, 4, 0)
    assert P.tobytes() == want[2].tobytes() and np.all(np.any(P[-2:] != 0, axis=1)) and P[-1, 3] != 0
    _check(a, before, got_before, want, "set_sliders behind added bodies")


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def _late_twins(ctx, cons_per_body, rows, every=False, traces=False):
    (a, b), scs, rig, u, planted = GR._late_twins(ctx, 2, cons_per_body_of_first=cons_per_body)
    lens = _lengths(a)
    sliders, W6 = LC.late_sliders(lens, a.state())
    hinges, HW6 = HC.late_hinges(lens, a.state())
    for t in (a, b):
        t.set_sliders(sliders)
        t.set_slider_targets(W6[:rows])
        if every or traces:
            t.set_hinges(hinges)
            t.set_hinge_targets(HW6[:2])
        if every:
            t.set_joints(JC.anchor_midpoints(JC.late_joints(lens, seed=431), a.state(), lens))
            t.set_springs(SP.late_springs(lens)[0])
        if traces:
            t.set_touches(XC.late_touch_rig())
            t.set_sensors(YC.late_sensor_rig())
            t.set_hinge_trace(RC.T, full=True)
    return a, b, scs, u, planted, sliders, W6[:rows]


def _rollout(a, U, dt, iters, mode, body, traces):
    """A's side: one call.  Returns (state traces as bytes by name, sensor rows, touch rows, stats bytes)"""
    if traces:
        return GS._observe(a, U, dt, iters, mode, body, touches="full")
    got, stats = GR._rollout(a, U, dt, iters, mode, body)
    return got, None, None, stats


def _loop(b, U, dt, iters, mode, body, traces, rows):
    """B's side: the defining loop, call by call - the sliders behind the hinges, tick t from row min(t, rows - 1).  With traces the
    hinge trace's row t is read back behind every tick as well (read_hinges_dev: the impulses are the handle's, of tick t's hinge solve)"""
    import torch
    ticks, m = len(U), len(body)
    out = GR._buffers(ticks, m)
    srows = GS._sensor_buffer(ticks, b.sensor_count()) if traces else None
    tb = GT._touch_buffer(ticks, b.touch_count()) if traces else None
    hr = torch.zeros((ticks, b.hinge_count(), 8), dtype=torch.float32, device="cuda") if traces else None
    ud, bd = GR._dev(U), GR._dev(body, np.int32)
    _sync()
    stats = b""
    for t in range(ticks):
        if b.spring_count():
            b.apply_springs_dev(dt)
        b.actuate_dev(ud[t], mode)
        if b.joint_count():
            b.solve_joints_dev(dt, iters)
        if b.hinge_count():
            b.solve_hinges_dev(dt, iters, min(t, 1))
        b.solve_sliders_dev(dt, iters, min(t, rows - 1))
        stats += bytes(b.step(dt, iters, 1))
        b.gather_state(bd, n=m, **{k: out[k][t] for k in out})
        if traces:
            b.read_touches_dev(tb[t])
            b.cast_sensors_dev(srows[t], kinds=GS.ALL)
            b.read_hinges_dev(hr[t])
    _sync()
    return ({k: out[k].cpu().numpy().tobytes() for k in out}, (GS._hit_rows(srows) if traces else None), (GT._rows(tb) if traces else None), stats,
            (hr.cpu().numpy() if traces else None))


@pytest.mark.parametrize("variant", ["alone_rows6", "all_rows3", "traces_rows1", "rerun_rows6"])
def test_a_rollout_with_sliders_is_the_defining_loop_also_when_ticks_are_run_again(ctx, variant):
    """alone: sliders alone, a table of 6 rows; all: with hinges, ball joints, springs and actuators (forces), a table of 3 - ticks 3..5
    read row 2; traces: with hinges and a touch trace, a sensor trace and a hinge trace, one row held for the whole call; rerun:
    cons_per_body = 1 - A's worlds outgrow their share in the MIDDLE of the rollout, so A's ticks are undone and run again while B never
    retries: sliders solved twice on a world that is run again, or not at all, show - a gate on `done` alone solves them twice"""
    import mgf_amd
    rerun, every, traces = variant.startswith("rerun"), "all" in variant, "traces" in variant
    rows = int(variant[-1])
    a, b, scs, u, planted, sliders, W = _late_twins(ctx, 1 if rerun else None, rows, every=every, traces=traces)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    T = RC.T
    assert T == 6 and W.shape == (rows, len(sliders)) and len(sliders) == 24
    U = RC.controls(u, planted, ticks=T)
    body, outside = RC.traced(len(a), count=30)
    mode = FORCE if every else IMPULSE
    got, srows, touches, got_stats = _rollout(a, U, dt, iters, mode, body, traces)
    launches = a.counter("rollout_launches")
    want, want_rows, want_touches, want_stats, want_hinges = _loop(b, U, dt, iters, mode, body, traces, rows)
    per_tick = (mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK + mgf_amd.BATCH_ROLLOUT_SLIDER_LAUNCHES_PER_TICK +
                (mgf_amd.BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK if every or traces else 0) +
                ((mgf_amd.BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK + mgf_amd.BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK) if every else 0) +
                ((mgf_amd.BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK + mgf_amd.BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK + mgf_amd.BATCH_ROLLOUT_HINGE_READ_LAUNCHES_PER_TICK) if traces else 0))
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
        tr = a.hinge_trace()
        assert tr.shape == (T, a.hinge_count()) and tr.view(np.float32).reshape(T, a.hinge_count(), 16)[:, :, :8].tobytes() == want_hinges.tobytes()
    assert not GR._same(a, b), GR._same(a, b)
    assert a.counter("sliders_skipped") == b.counter("sliders_skipped") == 0
    assert a.counter("actuators_skipped") == b.counter("actuators_skipped") == T * len(planted)
    # the sliders did something, and the table's rows did: a twin without the rig, and one whose table is row 0 alone, end elsewhere
    if not (every or traces):
        c = GR._late_twins(ctx, 1, cons_per_body_of_first=None)[0][0]
        plain, _ = GR._rollout(c, U, dt, iters, mode, body)
        assert plain["v"] != got["v"]
        e = GR._late_twins(ctx, 1, cons_per_body_of_first=None)[0][0]
        e.set_sliders(sliders)
        e.set_slider_targets(W[:1])
        held, _ = GR._rollout(e, U, dt, iters, mode, body)
        row = len(got["v"]) // T
        assert held["v"][:row] == got["v"][:row] and held["v"][row:] != got["v"][row:]             # tick 0 reads row 0 either way
        d1, off1, e1 = LC.travel(sliders, a.state(), _lengths(a))
        d0, off0, e0 = LC.travel(sliders, c.state(), _lengths(c))
        print("after", T, "ticks: largest off-axis gap and frame error with the sliders", off1.max(), e1.max(), "without", off0.max(), e0.max())


def test_the_launches_of_a_rollout_with_and_without_a_slider_rig(ctx):
    import mgf_amd
    import torch
    scs = RC.late_contact_scenes()
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    a, b, c, e, f = (mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True) for _ in range(5))
    lens = _lengths(a)
    sliders, W6 = LC.late_sliders(lens, a.state())
    for t in (a, b):
        t.set_sliders(sliders)
        t.set_slider_targets(W6[:2])
    # no controls and no traces, a slider rig that is not empty: NOT mgf_batch_step, but the loop solve_sliders_dev | step(1)
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    st = a.rollout_dev(RC.T, dt, iters, body=none)
    assert a.counter("rollout_launches") == RC.T * (mgf_amd.BATCH_ROLLOUT_SLIDER_LAUNCHES_PER_TICK + 1)     # and the launch that moves `act`
    stats = b""
    for t in range(RC.T):
        b.solve_sliders_dev(dt, iters, min(t, 1))
        assert b.counter("drive_launches") == mgf_amd.BATCH_SLIDER_LAUNCHES
        stats += bytes(b.step(dt, iters, 1))
    assert bytes(st) == stats and not GR._same(a, b)
    c.step(dt, iters, RC.T)
    assert GR._same(a, c)                                                       # it differs from step(T) ...
    a.step(dt, iters, 2)                                                        # ... which applies no slider, with or without a rig
    for _ in range(2):
        b.step(dt, iters, 1)
    assert not GR._same(a, b)
    # the host form is the device form
    a.rollout(RC.T, dt, iters, trace=())
    b.rollout_dev(RC.T, dt, iters, body=none)
    assert not GR._same(a, b)
    # an empty slider rig beside a hinge rollout: the same bytes and the same launches as on a batch that never had one
    hinges, HW6 = HC.late_hinges(lens, e.state())
    body, _ = RC.traced(len(e), count=10)
    e.set_sliders(sliders)
    e.set_slider_targets(W6)
    e.set_sliders(sliders[:0])                                                  # set and cleared: empty
    for t in (e, f):
        t.set_hinges(hinges)
        t.set_hinge_targets(HW6)
    ge, se = GR._rollout(e, RC.T, dt, iters, IMPULSE, body, T=RC.T)
    gf, sf = GR._rollout(f, RC.T, dt, iters, IMPULSE, body, T=RC.T)
    assert ge == gf and se == sf and not GR._same(e, f) and e.slider_count() == 0
    parent = f.counter("rollout_launches")
    assert e.counter("rollout_launches") == parent == RC.T * (1 + mgf_amd.BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK)
    e.set_sliders(sliders)
    GR._rollout(e, RC.T, dt, iters, IMPULSE, body, T=RC.T)
    assert e.counter("rollout_launches") == parent + RC.T and e.counter("capacity_retries") == 0


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
# what the float64 restatement with a stand-in tick shows on the CPU (LC.lift_sim(True), printed by the test below): the welded body's
# largest anchor gap and frame error over the 64 ticks.  The GPU's may be 8 times that, the host test's convention.
WELD_GAP_CPU = 8.91e-4
WELD_TILT_CPU = 5.2e-5


def test_a_limited_lift_stays_in_its_range_and_a_welded_body_keeps_its_pose_through_the_real_tick(ctx):
    """A body on a vertical slider to the world under gravity - the scene's force rows -, limited to [-0.3, 0.4], a second body welded
    to it by LOCK; 64 ticks of a rollout that traces x, q, v and omega; d from the trace in float64.  A limit acts from the call after
    the travel passed it, so one tick's travel is the definition's own overshoot: d must stay within the range widened by twice the
    largest |rate| * dt of that trace.  The same rollout with the LIMIT flag cleared must leave the range by more than ten times that
    margin.  The float64 restatement with a stand-in tick does both on the CPU - asserted here first - and gives the bounds of the weld."""
    import mgf_amd
    sc = LC.lift_scene()
    dt = float(sc["dt"])
    d, rate, gap, tilt = LC.lift_sim(True)
    inside, out, margin = LC.lift_verdict(d, rate, dt)
    free = LC.lift_verdict(*LC.lift_sim(False)[:2], dt)
    print("CPU: with the limit d leaves the range by", out, "margin", margin, "; without by", free[1], "; weld: gap", gap.max(), "frame error", tilt.max())
    assert inside and free[1] > 10 * margin
    assert gap.max() <= WELD_GAP_CPU * 1.01 and tilt.max() <= WELD_TILT_CPU * 1.01
    results = []
    for limit in (True, False):
        b = mgf_amd.WorldBatch.from_scenes(ctx, [sc], own_terrain=True)
        rig = LC.lift_rig(b.state(), limit)
        b.set_sliders(rig)
        tr = b.rollout(LC.LIFT_TICKS, dt, LC.LIFT_ITERS, trace=("x", "q", "v", "omega"))
        assert b.counter("sliders_skipped") == 0
        d, rate, gap, tilt = LC.lift_trace(rig, tr["x"], tr["q"], tr["v"], tr["omega"])
        results.append(LC.lift_verdict(d, rate, dt) + (float(d.min()), float(d.max()), float(gap.max()), float(tilt.max())))
    (inside, out, margin, lo, hi, gap, tilt), free = results
    print("GPU: with the limit d in [%.4f, %.4f], leaves the range by %.4f, margin %.4f; weld: gap %.2e, frame error %.2e; without the limit d leaves by %.4f"
          % (lo, hi, out, margin, gap, tilt, free[1]))
    assert inside, (out, margin)
    assert free[1] > 10 * margin, (free[1], margin)
    assert hi > LC.LIFT_LIMIT[1] - 0.05                                         # the limit was reached: it is what held the lift
    assert gap <= 8 * WELD_GAP_CPU and tilt <= 8 * WELD_TILT_CPU, (gap, tilt)
