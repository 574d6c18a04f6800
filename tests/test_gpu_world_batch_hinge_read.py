"""The hinge encoders of a batch (mgf_batch_read_hinges / _read_hinges_dev / _set_hinge_trace / _hinge_trace_rows / _get_hinge_trace /
_get_hinge_trace_dev; WorldBatch.read_hinges / .read_hinges_dev / .set_hinge_trace / .hinge_trace_rows / .hinge_trace / .hinge_trace_dev)
against their definition: a read equals the numpy restatement over state() byte for byte (tests/batch_hinge_read_cases.py) through both
forms - three worlds, one of them without hinges and one of bodies of several components, 0, 1 and 257 hinges, both kinds of far end,
the limit off, on and inside, past lo and past hi, pending host-side state - and touches nothing; the readings table of a rollout equals
the rows of the defining loop  ... | solve_hinges_dev | step(1) | gather_state | read_hinges_dev(row t)  by bytes through every rollout
form, both formats and every relation of rows to ticks - also when ticks are undone and run again; the launches; the refusals; and the
limited elbow of tests/batch_hinge_cases.py felt through the trace."""
import numpy as np
import pytest

from tests import batch_actuator_cases as AC
from tests import batch_hinge_cases as HC
from tests import batch_hinge_read_cases as HR
from tests import batch_rollout_cases as RC
from tests import batch_scan_cases as YC
from tests import batch_trace_cases as XC
from tests import test_gpu_world_batch_rollout as GR

pytestmark = pytest.mark.gpu
IMPULSE = AC.IMPULSE
FILL = 0x5A5A5A5A
T = 4
ENTRIES = ("rollout", "rollout_touches", "rollout_observe")


@pytest.fixture(scope="module")
def ctx():
    import mgf_amd
    c = mgf_amd.Context(0)
    yield c
    c.close()


_sync, _lengths = GR._sync, GR._lengths


def _fill(*shape):
    import torch
    return torch.full(shape, FILL, dtype=torch.int32, device="cuda").view(torch.float32)


# ---- the call ---------------------------------------------------------------------------------------------------------------------------------
def _batch(ctx):
    """three worlds - dumbbells and spheres (bodies of several components), 18 spheres, 27 spheres - ticked, then q, v and omega written
    into every body: every frame turned, every rate live"""
    import mgf_amd
    from tests import batch_parts_cases as PC
    late = RC.late_contact_scenes()
    scs = [PC.six_scenes()[PC.DUMBBELLS], late[RC.LATE_B], late[RC.LATE_A]]
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    b.step(float(scs[0]["dt"]), scs[0]["iters"], 2)
    q, v, om = HC.written_state(len(b))
    b.write_state(None, q=q, v=v, omega=om)
    return b


def _read_dev(b):
    """read_hinges_dev between two waits for the whole device; the array starts as 0x5A bytes: a word the call does not write shows"""
    out = _fill(b.hinge_count(), 8)
    _sync()
    b.read_hinges_dev(out)
    launches = b.counter("drive_launches")
    _sync()
    return out.cpu().numpy(), launches


@pytest.mark.parametrize("n", [0, 1, 257])
def test_a_read_is_the_restatement_by_bytes_through_both_forms_and_touches_nothing(ctx, n):
    import mgf_amd
    b = _batch(ctx)
    lens = _lengths(b)
    assert len(lens) == 3 and b.counter("launches_per_tick") == 7                # bodies of several components are present
    rig, case = HR.small_rig(lens, b.state(), n, worlds=(0, 2))                  # world 1 has no hinge
    b.set_hinges(rig)
    assert b.hinge_count() == n and 1 not in rig["world"]
    if n == 257:
        assert np.bincount(rig["world"]).tolist() == [129, 0, 128] and set(case) == {0, 1, 2, 3} and {-1} < set(rig["other"].tolist())
    st = b.state()
    want = HR.readings(rig, st, lens)
    kept = GR._everything(b)
    got = b.read_hinges()                                                        # the host form
    assert b.counter("drive_launches") == (1 if n else 0) and mgf_amd.BATCH_HINGE_READ_LAUNCHES == 1
    assert got.dtype == mgf_amd.HINGE_READING_DTYPE and got.shape == (n,)
    assert HR.words(got).tobytes() == want.tobytes(), HR.where(HR.words(got), want)
    got_dev, launches = _read_dev(b)                                             # the device form
    assert launches == (1 if n else 0) and got_dev.tobytes() == want.tobytes(), HR.where(got_dev, want)
    assert GR._everything(b) == kept                                             # the state is byte for byte as it was
    if n == 0:
        b.read_hinges_dev(None)
        return
    assert [float(s) for s in got["side"]] == [HR.SIDE_OF[HR.LIMIT_CASES[c]] for c in case]
    assert np.all(np.isfinite(want)) and np.all(got["tilt2"] > 0) and np.all(got["tilt2"] < 0.0101) and np.any(got["rate"] != 0)
    th, rate = mgf_amd.hinge_angles(got)
    d = np.abs((th - HC.thetas(rig, st, lens) + np.pi) % (2 * np.pi) - np.pi)
    print("n =", n, ": largest |theta - float64 theta|", d.max(), "bound", HR.THETA_BOUND)
    assert d.max() <= HR.THETA_BOUND
    # a read straight after set_many, without a step: the pending state goes up first
    off = np.concatenate([[0], np.cumsum(lens)])
    w, bd = rig["world"][:1], rig["body"][:1]
    ga = int(off[w[0]] + bd[0])
    st2 = {k: a.copy() for k, a in st.items()}
    st2["v"][ga], st2["omega"][ga] = (0.5, -1.0, 2.0), (3.0, -4.0, 5.5)
    b.set_velocities(w, bd, st2["v"][ga:ga + 1], st2["omega"][ga:ga + 1])
    want2 = HR.readings(rig, st2, lens)
    got2 = HR.words(b.read_hinges())
    assert want2.tobytes() != want.tobytes() and got2.tobytes() == want2.tobytes(), HR.where(got2, want2)
    assert b.state()["omega"].tobytes() == st2["omega"].tobytes()
    # a NaN pose gives NaN words and no error; every hinge that does not name the body reads as before
    q = st2["q"].copy()
    q[ga] = np.nan
    b.write_state(None, q=q)
    got3 = HR.words(b.read_hinges())
    names = (off[rig["world"]] + rig["body"] == ga) | ((rig["other"] >= 0) & (off[rig["world"]] + rig["other"] == ga))
    assert names[0] and np.isnan(got3[names][:, [0, 1, 7]]).all() and np.all(got3[names][:, 3] == 0)
    assert got3[~names].tobytes() == want2[~names].tobytes()


def test_refusals_enqueue_nothing_and_leave_the_table_the_rig_and_the_state_as_they_were(ctx):
    import mgf_amd
    import torch
    from mgf_amd import _capi
    INV = _capi.ERR_INVALID
    b = _batch(ctx)
    lens = _lengths(b)
    rig, case = HR.small_rig(lens, b.state(), 9, worlds=(0, 2))
    b.set_hinges(rig)
    n = len(rig)
    lib = mgf_amd.load_library()

    def err():
        return lib.mgf_last_error().decode()
    b.set_hinge_trace(3, full=True)
    assert b.hinge_trace_rows() == 3
    b.rollout(2, 1.0 / 60.0, 4, trace=())                                       # rows 0 and 1 of the table are written
    table = b.hinge_trace()
    assert table.shape == (3, n) and table.dtype == mgf_amd.HINGE_TRACE_FULL_DTYPE and HR.words(table[:2]).any() and not HR.words(table[2:]).any()
    kept = GR._everything(b)
    out = np.zeros((n, 8), np.float32)
    dev = torch.zeros(16 * 3 * n + 8, dtype=torch.float32, device="cuda")
    _sync()
    b.read_hinges()
    assert b.counter("drive_launches") == 1
    assert lib.mgf_batch_read_hinges(b._h, None) == INV and "NULL argument: out" in err()
    assert lib.mgf_batch_read_hinges_dev(b._h, None) == INV and "NULL argument: out" in err()
    assert lib.mgf_batch_read_hinges_dev(b._h, dev.data_ptr() + 2) == INV and "aligned" in err()
    assert lib.mgf_batch_read_hinges_dev(b._h, dev.data_ptr() + 4) == INV and "aligned to 16" in err()
    assert lib.mgf_batch_read_hinges_dev(b._h, out.ctypes.data) == INV and "device memory" in err()
    assert b.counter("drive_launches") == 0                                      # behind a refused call
    for rows in (-1, (1 << 20) + 1):
        assert lib.mgf_batch_set_hinge_trace(b._h, rows, 9) == INV and "rows must be in [0, 2^20]" in err()
    for fmt in (-1, 2):
        assert lib.mgf_batch_set_hinge_trace(b._h, 5, fmt) == INV and "format is neither" in err()
    big = np.zeros((3, n, 16), np.float32)
    for row0, n_rows, word in ((-1, 1, "row0 is negative"), (0, -1, "n_rows is negative"), (-1, -1, "row0 is negative"), (0, 4, "beyond"), (3, 1, "beyond"), (1 << 40, 0, "beyond")):
        assert lib.mgf_batch_get_hinge_trace(b._h, big.ctypes.data, row0, n_rows) == INV and word in err(), (row0, n_rows)
        assert lib.mgf_batch_get_hinge_trace_dev(b._h, dev.data_ptr(), row0, n_rows) == INV and word in err(), (row0, n_rows)
    assert lib.mgf_batch_get_hinge_trace(b._h, None, 0, 1) == INV and "NULL argument: out" in err()
    assert lib.mgf_batch_get_hinge_trace_dev(b._h, None, 1, 2) == INV and "NULL argument: out" in err()
    assert lib.mgf_batch_get_hinge_trace_dev(b._h, dev.data_ptr() + 2, 0, 3) == INV and "aligned" in err()
    assert lib.mgf_batch_get_hinge_trace_dev(b._h, big.ctypes.data, 0, 3) == INV and "device memory" in err()
    assert lib.mgf_batch_get_hinge_trace(b._h, None, 3, 0) == 0 and lib.mgf_batch_get_hinge_trace_dev(b._h, None, 0, 0) == 0    # nothing to copy
    _sync()
    assert not dev.any().item() and not out.any() and not big.any()              # nothing was written
    assert b.hinge_trace_rows() == 3 and b.hinge_count() == n and GR._everything(b) == kept
    assert b.hinge_trace().tobytes() == table.tobytes()                          # the table as it was
    part = torch.zeros((2 * n, 16), dtype=torch.float32, device="cuda")
    _sync()
    b.hinge_trace_dev(part, 1, 2)                                                # rows 1 and 2, device to device
    _sync()
    assert part.cpu().numpy().tobytes() == table[1:].tobytes() and b.hinge_trace(1, 1).tobytes() == table[1:2].tobytes()
    # an empty rig: MGF_OK, nothing enqueued; rows and format are kept
    e = _batch(ctx)
    e.set_hinge_trace(5)
    assert e.hinge_trace_rows() == 5 and e.hinge_trace().shape == (5, 0) and e.read_hinges().shape == (0,) and e.counter("drive_launches") == 0
    e.rollout(2, 1.0 / 60.0, 4, trace=())
    assert e.counter("rollout_launches") == 0                                    # no hinge: mgf_batch_step, launch for launch
    # set_hinges behind a trace turns it off; rows == 0 frees the table
    b.set_hinges(rig)
    assert b.hinge_trace_rows() == 0 and b.hinge_trace().shape == (0, n)
    b.set_hinge_trace(2)
    assert b.hinge_trace_rows() == 2 and not HR.words(b.hinge_trace()).any()     # allocated and zeroed
    b.set_hinge_trace(0)
    assert b.hinge_trace_rows() == 0
    assert lib.mgf_batch_get_hinge_trace(b._h, big.ctypes.data, 0, 1) == INV and "beyond" in err()


# ---- the rollouts -----------------------------------------------------------------------------------------------------------------------------
def _twins(ctx, cons_per_body):
    """twin batches of RC.late_contact_scenes() with the actuators', the hinges', the contact sensors' and the ray sensors' rigs and a
    target table of three rows; the first starts with cons_per_body = 1 where asked for: its ticks are undone and run again"""
    (a, b), scs, rig, u, planted = GR._late_twins(ctx, 2, cons_per_body_of_first=cons_per_body)
    lens = _lengths(a)
    hinges, W6 = HC.late_hinges(lens, a.state())
    for t in (a, b):
        t.set_hinges(hinges)
        t.set_hinge_targets(W6[:3])
        t.set_touches(XC.late_touch_rig())
        t.set_sensors(YC.late_sensor_rig())
    return a, b, scs, u, planted, hinges


def _rollout(a, entry, dev, U, dt, iters):
    """A's side: one call of `entry` in its host or device form, every body's q and omega traced.  Returns (q bytes, omega bytes)"""
    import torch
    ticks, m = len(U), len(a)
    if not dev:
        kw = {"rollout": {}, "rollout_touches": {}, "rollout_observe": dict(touches=True, sensors="hit")}[entry]
        tr = getattr(a, entry)(U, dt, iters, IMPULSE, trace=("q", "omega"), **kw)
        return tr["q"].tobytes(), tr["omega"].tobytes()
    q, om = _fill(ticks, m, 4), _fill(ticks, m, 3)
    kw = {}
    if entry != "rollout":
        kw["touches"] = torch.zeros((ticks, a.touch_count(), 16), dtype=torch.int32, device="cuda")
    if entry == "rollout_observe":
        kw["sensors"] = torch.zeros((ticks, a.sensor_count(), 7), dtype=torch.int32, device="cuda")
    _sync()
    getattr(a, entry + "_dev")(GR._dev(U), dt, iters, IMPULSE, q=q, omega=om, **kw)
    _sync()
    return q.cpu().numpy().tobytes(), om.cpu().numpy().tobytes()


def _table(a, dev):
    """A's table through the host or the device form of the get call, as float32 words [rows, n, 8 | 16]"""
    import torch
    if not dev:
        return HR.words(a.hinge_trace())
    rows, n = a.hinge_trace_rows(), a.hinge_count()
    cols = 16 if a._hinge_trace_full else 8
    out = _fill(rows * n, cols) if rows * n else torch.zeros((0, cols), dtype=torch.float32, device="cuda")
    _sync()                                                                      # (the fill runs on torch's stream, the copy on the context's)
    a.hinge_trace_dev(out)
    _sync()
    return out.cpu().numpy().reshape(rows, n, cols)


def _loop(b, U, dt, iters, table_rows, full, before):
    """B's side: the defining loop, call by call, with mgf_batch_read_hinges_dev(row t) at the end of every tick t < rows.  Returns
    (q bytes, omega bytes, the table the loop gives: `before` with the rows the loop reaches replaced)"""
    import torch
    ticks, m, n = len(U), len(b), b.hinge_count()
    q, om = _fill(ticks, m, 4), _fill(ticks, m, 3)
    reach = min(ticks, table_rows)
    rows = _fill(max(reach, 1), n, 8)
    imp = torch.zeros((ticks, n, 8), dtype=torch.float32, device="cuda")          # iters == 0: no solve is enqueued - zeros
    ud = GR._dev(U)
    _sync()
    for t in range(ticks):
        b.actuate_dev(ud[t], IMPULSE)
        b.solve_hinges_dev(dt, iters, min(t, 2), impulses_dev=imp[t])
        b.step(dt, iters, 1)
        b.gather_state(None, q=q[t], omega=om[t], n=m)
        if t < table_rows:
            b.read_hinges_dev(rows[t])
    _sync()
    want = before.copy()
    if reach:
        got = rows.cpu().numpy()[:reach]
        want[:reach] = np.concatenate([got, imp.cpu().numpy()[:reach]], axis=2) if full else got
    return q.cpu().numpy().tobytes(), om.cpu().numpy().tobytes(), want


def _per_tick(entry, iters):
    import mgf_amd
    return (mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK + (mgf_amd.BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK if iters else 0) +
            (mgf_amd.BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK if entry != "rollout" else 0) +
            (mgf_amd.BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK if entry == "rollout_observe" else 0))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_table_of_a_rollout_is_the_defining_loops_rows_by_bytes(ctx, entry, dev):
    """one pair of twins through a chain of rollouts of T = 4 ticks - rows 0, 1, 3, 4 and 6 in both formats, then iters == 0 - each from
    the state the last left: A takes one call, B the loop, and the table, the traced q and omega and the batches are compared by bytes"""
    import mgf_amd
    a, b, scs, u, planted, hinges = _twins(ctx, None)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    n = len(hinges)
    U = RC.controls(u, planted, ticks=T)
    assert n == 24 and mgf_amd.BATCH_ROLLOUT_HINGE_READ_LAUNCHES_PER_TICK == 1 and a.hinge_trace_rows() == 0
    for rows, full, its in [(r, f, iters) for f in (False, True) for r in (0, 1, 3, 4, 6)] + [(4, True, 0), (3, False, 0)]:
        a.set_hinge_trace(rows, full=full)
        cols = 16 if full else 8
        before = _table(a, dev)
        assert before.shape == (rows, n, cols) and not before.any() and a.hinge_trace_rows() == rows          # allocated and zeroed
        if rows == 6:                                                            # the rows a call of 4 ticks does not reach hold an earlier call's readings
            U6 = RC.controls(u, planted, ticks=6, seed=167)
            _rollout(a, entry, dev, U6, dt, its)
            assert a.counter("rollout_launches") == 6 * (_per_tick(entry, its) + 1)
            want6 = _loop(b, U6, dt, its, rows, full, before)[2]
            before = _table(a, dev)
            assert before.tobytes() == want6.tobytes() and before[4:].any()
        got_q, got_om = _rollout(a, entry, dev, U, dt, its)
        launches = a.counter("rollout_launches")
        assert a.counter("capacity_retries") == 0
        assert launches == T * _per_tick(entry, its) + min(T, rows), (rows, full, launches)                   # with rows == 0: what it is without the table
        want_q, want_om, want = _loop(b, U, dt, its, rows, full, before)
        got = _table(a, dev)
        assert got.tobytes() == want.tobytes(), (rows, full, its, HR.where(got, want))
        assert got_q == want_q and got_om == want_om and not GR._same(a, b), (rows, full, its)
        if rows:
            assert got[:min(T, rows), :, :8].any() and np.all(np.isfinite(got))
        if rows == 6:
            assert got[4:].tobytes() == before[4:].tobytes() and got[:4].tobytes() != before[:4].tobytes()    # rows >= T stay as they were
        if full and rows:
            reach = min(T, rows)
            assert (got[:reach, :, 8:11].any() and np.any(got[:reach, :, 14] != 0)) if its else not got[:, :, 8:].any()   # the point's and a motor's impulses; iters == 0: zeros
            assert not got[:, :, 15].any()
    assert a.counter("hinges_skipped") == b.counter("hinges_skipped")
    # set_hinges behind a trace turns it off: the rollout is launch for launch what it is without the table
    a.set_hinge_trace(4)
    a.set_hinges(hinges)
    assert a.hinge_trace_rows() == 0
    _rollout(a, entry, dev, U, dt, iters)
    assert a.counter("rollout_launches") == T * _per_tick(entry, iters)


RERUNS = [(e, d, (i + d) % 2 == 0, (6, 4)[(i + d) % 2], T) for i, e in enumerate(ENTRIES) for d in (False, True)] + [("rollout", True, True, 6, RC.T),
                                                                                                                   ("rollout_observe", False, False, 6, RC.T)]


@pytest.mark.parametrize("entry,dev,full,rows,ticks", RERUNS, ids=["%s-%s-%s-rows%d-T%d" % (e, "dev" if d else "host", "full" if f else "reading", r, t) for e, d, f, r, t in RERUNS])
def test_the_table_is_the_defining_loops_also_when_ticks_are_undone_and_run_again(ctx, entry, dev, full, rows, ticks):
    """cons_per_body = 1 - A's worlds outgrow their share in mid-call, so A's ticks are undone and run again while B never retries: a row
    written from the wrong pass, or the impulses of another tick's solve beside a reading, show.  T = 4: the last tick is run again;
    T = 6: ticks in the middle are, and later ticks of the earlier pass skip the undone world"""
    a, b, scs, u, planted, hinges = _twins(ctx, 1)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    U = RC.controls(u, planted, ticks=ticks)
    a.set_hinge_trace(rows, full=full)
    before = _table(a, dev)
    got_q, got_om = _rollout(a, entry, dev, U, dt, iters)
    launches = a.counter("rollout_launches")
    assert a.counter("capacity_retries") > 0 and launches > ticks * _per_tick(entry, iters) + min(ticks, rows)       # the re-run path was really taken
    want_q, want_om, want = _loop(b, U, dt, iters, rows, full, before)
    assert b.counter("capacity_retries") == 0
    got = _table(a, dev)
    reach = min(ticks, rows)
    assert got.tobytes() == want.tobytes(), [(t, HR.where(got[t], want[t])) for t in range(reach) if got[t].tobytes() != want[t].tobytes()]
    assert got_q == want_q and got_om == want_om and not GR._same(a, b)
    assert not got[reach:].any() and got[:reach, :, :8].any()


# ---- a use case ---------------------------------------------------------------------------------------------------------------------------------
def test_a_policy_feels_the_limited_elbow_through_the_trace(ctx):
    """tests/batch_hinge_cases.py's arm - the elbow limited to [-0.5, 0.7] - through 64 ticks of a rollout that traces q and omega and
    fills the readings table: hinge_angles of the traced readings equals arm_trace_angles of the traced q rows within THETA_BOUND (the
    rate within RATE_BOUND of |omega_a| + |omega_b|), and `side` is non-zero on exactly the ticks where that host angle lies outside
    the range - a tick whose angle is within THETA_BOUND of a limit is left out, at most 2 of 64."""
    import mgf_amd
    sc = HC.arm_scene()
    dt = float(sc["dt"])
    b = mgf_amd.WorldBatch.from_scenes(ctx, [sc], own_terrain=True)
    b.set_velocities([0, 0], [0, 1], sc["v0"], sc["omega0"])
    rig = HC.arm_rig(b.state(), True)
    b.set_hinges(rig)
    b.set_hinge_trace(HC.ARM_TICKS, full=True)
    tr = b.rollout(HC.ARM_TICKS, dt, HC.ARM_ITERS, trace=("q", "omega"))
    table = b.hinge_trace()
    assert table.shape == (HC.ARM_TICKS, 2) and b.counter("hinges_skipped") == 0
    theta, rate = mgf_amd.hinge_angles(table[:, 1])
    want_theta, want_rate = HC.arm_trace_angles(rig, tr["q"], tr["omega"])
    scale = np.linalg.norm(tr["omega"][:, 0].astype(np.float64), axis=1) + np.linalg.norm(tr["omega"][:, 1].astype(np.float64), axis=1)
    print("the elbow: largest |theta - host theta| %.3g rad (bound %.3g), |rate - host rate| / (|omega_a| + |omega_b|) %.3g (bound %.3g)"
          % (np.abs(theta - want_theta).max(), HR.THETA_BOUND, (np.abs(rate - want_rate) / scale).max(), HR.RATE_BOUND))
    assert np.abs(theta - want_theta).max() <= HR.THETA_BOUND
    assert np.all(np.abs(rate - want_rate) <= HR.RATE_BOUND * scale)
    lo, hi = HC.ARM_LIMIT
    near = np.minimum(np.abs(want_theta - lo), np.abs(want_theta - hi)) <= HR.THETA_BOUND
    print("ticks within the bound of a limit:", int(near.sum()), "; the nearest is", float(np.minimum(np.abs(want_theta - lo), np.abs(want_theta - hi)).min()), "rad from it")
    assert int(near.sum()) <= 2
    outside = (want_theta < lo) | (want_theta > hi)
    side = table["side"][:, 1]
    assert np.array_equal((side != 0)[~near], outside[~near]), np.flatnonzero((side != 0) != outside)
    assert np.all(side[(want_theta < lo) & ~near] == -1.0) and np.all(side[(want_theta > hi) & ~near] == 1.0) and outside.any() and not outside.all()
    assert not table["side"][:, 0].any()                                         # the shoulder has no limit
    # the limit's impulse beside the reading: it acts in the tick after a reading that says so, never behind one that says the row is off
    al = table["al"][:, 1]
    assert not al[1:][side[:-1] == 0].any() and not al[0] and np.all(al[1:][side[:-1] < 0] >= 0) and np.any(al > 0)
    print("anchor gap at most %.3g, tilt2 at most %.3g over the rollout" % (np.linalg.norm(table["gap"], axis=2).max(), table["tilt2"].max()))
