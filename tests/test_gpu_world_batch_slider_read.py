"""The slider encoders of a batch (mgf_batch_read_sliders / _read_sliders_dev / _set_slider_trace / _slider_trace_rows / _get_slider_trace /
_get_slider_trace_dev; WorldBatch.read_sliders / .read_sliders_dev / .set_slider_trace / .slider_trace_rows / .slider_trace /
.slider_trace_dev) against their definition: a read equals the numpy restatement over state() byte for byte
(tests/batch_slider_read_cases.py) through both forms - three worlds, one of them without sliders and one of bodies of several
components, 0, 1 and 257 sliders, both kinds of far end, every flag case, pending host-side state - and touches nothing; the readings
table of a rollout equals the rows of the defining loop  ... | solve_sliders_dev | step(1) | gather_state | read_sliders_dev(row t)  by
bytes through every rollout form, both formats and every relation of rows to ticks - also beside a hinge trace, and when ticks are
undone and run again; the launches; the refusals; and the limited lift of tests/batch_slider_cases.py felt through the trace."""
import numpy as np
import pytest

from tests import batch_actuator_cases as AC
from tests import batch_hinge_cases as HC
from tests import batch_hinge_read_cases as HR
from tests import batch_rollout_cases as RC
from tests import batch_scan_cases as YC
from tests import batch_slider_cases as LC
from tests import batch_slider_read_cases as SR
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
    q, v, om = LC.written_state(len(b))
    b.write_state(None, q=q, v=v, omega=om)
    return b


def _read_dev(b):
    """read_sliders_dev between two waits for the whole device; the array starts as 0x5A bytes: a word the call does not write shows"""
    out = _fill(b.slider_count(), 8)
    _sync()
    b.read_sliders_dev(out)
    launches = b.counter("drive_launches")
    _sync()
    return out.cpu().numpy(), launches


@pytest.mark.parametrize("n", [0, 1, 257])
def test_a_read_is_the_restatement_by_bytes_through_both_forms_and_touches_nothing(ctx, n):
    import mgf_amd
    b = _batch(ctx)
    lens = _lengths(b)
    assert len(lens) == 3 and b.counter("launches_per_tick") == 7                # bodies of several components are present
    rig, case = SR.small_rig(lens, b.state(), n, worlds=(0, 2))                  # world 1 has no slider
    b.set_sliders(rig)
    assert b.slider_count() == n and 1 not in rig["world"]
    if n == 257:                                                                 # 257 lanes: one in a second workgroup
        assert np.bincount(rig["world"]).tolist() == [129, 0, 128] and set(case) == set(range(len(SR.CASES))) and {-1} < set(rig["other"].tolist())
    st = b.state()
    want = SR.readings(rig, st, lens)
    kept = GR._everything(b)
    got = b.read_sliders()                                                       # the host form
    assert b.counter("drive_launches") == (1 if n else 0) and mgf_amd.BATCH_SLIDER_READ_LAUNCHES == 1
    assert got.dtype == mgf_amd.SLIDER_READING_DTYPE and got.shape == (n,)
    assert SR.words(got).tobytes() == want.tobytes(), SR.where(SR.words(got), want)
    got_dev, launches = _read_dev(b)                                             # the device form
    assert launches == (1 if n else 0) and got_dev.tobytes() == want.tobytes(), SR.where(got_dev, want)
    assert GR._everything(b) == kept                                             # state(), get() and the constraint lists are byte for byte as they were
    if n == 0:
        b.read_sliders_dev(None)
        return
    assert [float(s) for s in got["side"]] == [SR.SIDE_OF[SR.CASES[c]] for c in case]
    assert np.all(np.isfinite(want)) and np.any(got["rate"] != 0) and np.any(got["off"] != 0) and np.any(got["e"] != 0)
    r64 = SR.readings(rig, st, lens, np.float64)                                # the float64 reading of the same state: the bounds' reference
    bd, bo, be, br = SR.bounds(rig, st, lens)
    diff = np.abs(SR.words(got).astype(np.float64) - r64)
    print("n =", n, ": largest differences from the float64 reading as shares of their bounds: d", (diff[:, 0] / bd).max(), "off", (diff[:, 3:5].max(axis=1) / bo).max(),
          "e", (diff[:, 5:8].max(axis=1) / be).max(), "rate", (diff[:, 1] / br).max(), "; largest d bound", bd.max())
    assert np.all(diff[:, 0] <= bd) and np.all(diff[:, 3:5].max(axis=1) <= bo) and np.all(diff[:, 5:8].max(axis=1) <= be) and np.all(diff[:, 1] <= br)
    # a read straight after set_velocities, without a step: the pending state goes up first
    off = np.concatenate([[0], np.cumsum(lens)])
    w, bd_ = rig["world"][:1], rig["body"][:1]
    ga = int(off[w[0]] + bd_[0])
    st2 = {k: a.copy() for k, a in st.items()}
    st2["v"][ga], st2["omega"][ga] = (0.5, -1.0, 2.0), (3.0, -4.0, 5.5)
    b.set_velocities(w, bd_, st2["v"][ga:ga + 1], st2["omega"][ga:ga + 1])
    want2 = SR.readings(rig, st2, lens)
    got2 = SR.words(b.read_sliders())
    assert want2.tobytes() != want.tobytes() and got2.tobytes() == want2.tobytes(), SR.where(got2, want2)
    assert want2[0, 1] != want[0, 1] and want2[0, 0] == want[0, 0]               # the rate moved, the travel did not
    assert b.state()["v"].tobytes() == st2["v"].tobytes() and b.state()["omega"].tobytes() == st2["omega"].tobytes()
    # a NaN pose gives NaN words and no error; every slider that does not name the body reads as before
    q = st2["q"].copy()
    q[ga] = np.nan
    b.write_state(None, q=q)
    got3 = SR.words(b.read_sliders())
    names = (off[rig["world"]] + rig["body"] == ga) | ((rig["other"] >= 0) & (off[rig["world"]] + rig["other"] == ga))
    assert names[0] and np.isnan(got3[names][:, [0, 1, 3, 4, 5, 6, 7]]).all()
    assert np.all(got3[names][:, 2] == np.where(rig["flags"][names] & LC.LOCK, 2.0, 0.0))
    assert got3[~names].tobytes() == want2[~names].tobytes()


def test_refusals_enqueue_nothing_and_leave_the_table_the_rig_and_the_state_as_they_were(ctx):
    import mgf_amd
    import torch
    from mgf_amd import _capi
    INV = _capi.ERR_INVALID
    b = _batch(ctx)
    lens = _lengths(b)
    rig, case = SR.small_rig(lens, b.state(), 9, worlds=(0, 2))
    b.set_sliders(rig)
    n = len(rig)
    lib = mgf_amd.load_library()

    def err():
        return lib.mgf_last_error().decode()
    b.set_slider_trace(3, full=True)
    assert b.slider_trace_rows() == 3
    b.rollout(2, 1.0 / 60.0, 4, trace=())                                       # rows 0 and 1 of the table are written
    table = b.slider_trace()
    assert table.shape == (3, n) and table.dtype == mgf_amd.SLIDER_TRACE_FULL_DTYPE and SR.words(table[:2]).any() and not SR.words(table[2:]).any()
    kept = GR._everything(b)
    out = np.zeros((n, 8), np.float32)
    dev = torch.zeros(16 * 3 * n + 8, dtype=torch.float32, device="cuda")
    _sync()
    b.read_sliders()
    assert b.counter("drive_launches") == 1
    assert lib.mgf_batch_read_sliders(b._h, None) == INV and "NULL argument: out" in err()
    assert lib.mgf_batch_read_sliders_dev(b._h, None) == INV and "NULL argument: out" in err()
    assert lib.mgf_batch_read_sliders_dev(b._h, dev.data_ptr() + 2) == INV and "aligned" in err()
    assert lib.mgf_batch_read_sliders_dev(b._h, dev.data_ptr() + 4) == INV and "aligned to 16" in err()
    assert lib.mgf_batch_read_sliders_dev(b._h, out.ctypes.data) == INV and "device memory" in err()
    assert b.counter("drive_launches") == 0                                      # behind a refused call
    for rows in (-1, (1 << 20) + 1):
        assert lib.mgf_batch_set_slider_trace(b._h, rows, 9) == INV and "rows must be in [0, 2^20]" in err()
    for fmt in (-1, 2):
        assert lib.mgf_batch_set_slider_trace(b._h, 5, fmt) == INV and "format is neither" in err()
    big = np.zeros((3, n, 16), np.float32)
    for row0, n_rows, word in ((-1, 1, "row0 is negative"), (0, -1, "n_rows is negative"), (-1, -1, "row0 is negative"), (0, 4, "beyond"), (3, 1, "beyond"), (1 << 40, 0, "beyond")):
        assert lib.mgf_batch_get_slider_trace(b._h, big.ctypes.data, row0, n_rows) == INV and word in err(), (row0, n_rows)
        assert lib.mgf_batch_get_slider_trace_dev(b._h, dev.data_ptr(), row0, n_rows) == INV and word in err(), (row0, n_rows)
    assert lib.mgf_batch_get_slider_trace(b._h, None, 0, 1) == INV and "NULL argument: out" in err()
    assert lib.mgf_batch_get_slider_trace_dev(b._h, None, 1, 2) == INV and "NULL argument: out" in err()
    assert lib.mgf_batch_get_slider_trace_dev(b._h, dev.data_ptr() + 2, 0, 3) == INV and "aligned" in err()
    assert lib.mgf_batch_get_slider_trace_dev(b._h, big.ctypes.data, 0, 3) == INV and "device memory" in err()
    assert lib.mgf_batch_get_slider_trace(b._h, None, 3, 0) == 0 and lib.mgf_batch_get_slider_trace_dev(b._h, None, 0, 0) == 0    # nothing to copy
    _sync()
    assert not dev.any().item() and not out.any() and not big.any()              # nothing was written
    assert b.slider_trace_rows() == 3 and b.slider_count() == n and GR._everything(b) == kept
    assert b.slider_trace().tobytes() == table.tobytes()                         # the table as it was
    part = torch.zeros((2 * n, 16), dtype=torch.float32, device="cuda")
    _sync()
    b.slider_trace_dev(part, 1, 2)                                               # rows 1 and 2, device to device
    _sync()
    assert part.cpu().numpy().tobytes() == table[1:].tobytes() and b.slider_trace(1, 1).tobytes() == table[1:2].tobytes()
    # an empty rig: MGF_OK, nothing enqueued; rows and format are kept
    e = _batch(ctx)
    e.set_slider_trace(5)
    assert e.slider_trace_rows() == 5 and e.slider_trace().shape == (5, 0) and e.read_sliders().shape == (0,) and e.counter("drive_launches") == 0
    e.rollout(2, 1.0 / 60.0, 4, trace=())
    assert e.counter("rollout_launches") == 0                                    # no slider: mgf_batch_step, launch for launch
    # set_sliders behind a trace turns it off; rows == 0 frees the table
    b.set_sliders(rig)
    assert b.slider_trace_rows() == 0 and b.slider_trace().shape == (0, n)
    b.set_slider_trace(2)
    assert b.slider_trace_rows() == 2 and not SR.words(b.slider_trace()).any()   # allocated and zeroed
    b.set_slider_trace(0)
    assert b.slider_trace_rows() == 0
    assert lib.mgf_batch_get_slider_trace(b._h, big.ctypes.data, 0, 1) == INV and "beyond" in err()


# ---- the rollouts -----------------------------------------------------------------------------------------------------------------------------
def _twins(ctx, cons_per_body):
    """twin batches of RC.late_contact_scenes() with the actuators', the sliders', the contact sensors' and the ray sensors' rigs and a
    target table of three rows; the first starts with cons_per_body = 1 where asked for: its ticks are undone and run again"""
    (a, b), scs, rig, u, planted = GR._late_twins(ctx, 2, cons_per_body_of_first=cons_per_body)
    lens = _lengths(a)
    sliders, W6 = LC.late_sliders(lens, a.state())
    for t in (a, b):
        t.set_sliders(sliders)
        t.set_slider_targets(W6[:3])
        t.set_touches(XC.late_touch_rig())
        t.set_sensors(YC.late_sensor_rig())
    return a, b, scs, u, planted, sliders


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


def _table(a, dev, hinge=False):
    """A's table - the sliders', or the hinges' - through the host or the device form of the get call, as float32 words [rows, n, 8 | 16]"""
    import torch
    word = "hinge" if hinge else "slider"
    if not dev:
        return SR.words(getattr(a, word + "_trace")())
    rows, n = getattr(a, word + "_trace_rows")(), getattr(a, word + "_count")()
    cols = 16 if getattr(a, "_%s_trace_full" % word) else 8
    out = _fill(rows * n, cols) if rows * n else torch.zeros((0, cols), dtype=torch.float32, device="cuda")
    _sync()                                                                      # (the fill runs on torch's stream, the copy on the context's)
    getattr(a, word + "_trace_dev")(out)
    _sync()
    return out.cpu().numpy().reshape(rows, n, cols)


def _loop(b, U, dt, iters, table_rows, full, before, hinge_rows=0, hinge_before=None):
    """B's side: the defining loop, call by call, with mgf_batch_read_sliders_dev(row t) at the end of every tick t < rows - behind
    mgf_batch_read_hinges_dev(row t) where B has hinges and t < hinge_rows.  Returns (q bytes, omega bytes, the table the loop gives:
    `before` with the rows the loop reaches replaced, and the hinges' full table likewise)"""
    import torch
    ticks, m, n, nh = len(U), len(b), b.slider_count(), b.hinge_count()
    q, om = _fill(ticks, m, 4), _fill(ticks, m, 3)
    reach, hreach = min(ticks, table_rows), min(ticks, hinge_rows)
    rows, hrows = _fill(max(reach, 1), n, 8), _fill(max(hreach, 1), max(nh, 1), 8)
    imp = torch.zeros((ticks, n, 8), dtype=torch.float32, device="cuda")          # iters == 0: no solve is enqueued - zeros
    himp = torch.zeros((ticks, max(nh, 1), 8), dtype=torch.float32, device="cuda")
    ud = GR._dev(U)
    _sync()
    for t in range(ticks):
        b.actuate_dev(ud[t], IMPULSE)
        if nh:
            b.solve_hinges_dev(dt, iters, min(t, 2), impulses_dev=himp[t])
        b.solve_sliders_dev(dt, iters, min(t, 2), impulses_dev=imp[t])
        b.step(dt, iters, 1)
        b.gather_state(None, q=q[t], omega=om[t], n=m)
        if nh and t < hinge_rows:
            b.read_hinges_dev(hrows[t])
        if t < table_rows:
            b.read_sliders_dev(rows[t])
    _sync()
    want = before.copy()
    if reach:
        got = rows.cpu().numpy()[:reach]
        want[:reach] = np.concatenate([got, imp.cpu().numpy()[:reach]], axis=2) if full else got
    hwant = None
    if hinge_before is not None:
        hwant = hinge_before.copy()
        hwant[:hreach] = np.concatenate([hrows.cpu().numpy()[:hreach], himp.cpu().numpy()[:hreach]], axis=2)
    return q.cpu().numpy().tobytes(), om.cpu().numpy().tobytes(), want, hwant


def _per_tick(entry, iters, hinges=False):
    import mgf_amd
    return (mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK + (mgf_amd.BATCH_ROLLOUT_SLIDER_LAUNCHES_PER_TICK if iters else 0) +
            (mgf_amd.BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK if iters and hinges else 0) +
            (mgf_amd.BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK if entry != "rollout" else 0) +
            (mgf_amd.BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK if entry == "rollout_observe" else 0))


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_table_of_a_rollout_is_the_defining_loops_rows_by_bytes(ctx, entry, dev):
    """one pair of twins through a chain of rollouts of T = 4 ticks - rows 0, 1, 3, 4 and 6 in both formats, then iters == 0, then beside a
    hinge trace - each from the state the last left: A takes one call, B the loop, and the table, the traced q and omega and the batches
    are compared by bytes"""
    import mgf_amd
    a, b, scs, u, planted, sliders = _twins(ctx, None)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    n = len(sliders)
    U = RC.controls(u, planted, ticks=T)
    assert n == 24 and mgf_amd.BATCH_ROLLOUT_SLIDER_READ_LAUNCHES_PER_TICK == 1 and a.slider_trace_rows() == 0
    for rows, full, its in [(r, f, iters) for f in (False, True) for r in (0, 1, 3, 4, 6)] + [(4, True, 0), (3, False, 0)]:
        a.set_slider_trace(rows, full=full)
        cols = 16 if full else 8
        before = _table(a, dev)
        assert before.shape == (rows, n, cols) and not before.any() and a.slider_trace_rows() == rows         # allocated and zeroed
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
        want_q, want_om, want, _ = _loop(b, U, dt, its, rows, full, before)
        got = _table(a, dev)
        assert got.tobytes() == want.tobytes(), (rows, full, its, SR.where(got, want))
        assert got_q == want_q and got_om == want_om and not GR._same(a, b), (rows, full, its)
        if rows:
            assert got[:min(T, rows), :, :8].any() and np.all(np.isfinite(got))
        if rows == 6:
            assert got[4:].tobytes() == before[4:].tobytes() and got[:4].tobytes() != before[:4].tobytes()    # rows >= T stay as they were
        if full and rows:
            reach = min(T, rows)
            assert (got[:reach, :, 8:10].any() and np.any(got[:reach, :, 11] != 0) and got[:reach, :, 12:15].any()) if its else not got[:, :, 8:].any()   # the off-axis, a motor's and the angular impulses; iters == 0: zeros
            assert not got[:, :, 15].any()
    assert a.counter("sliders_skipped") == b.counter("sliders_skipped")
    # beside a hinge trace: both tables are filled, the hinges' behind tick t first, and the count grows by both
    hinges, HW6 = HC.late_hinges(_lengths(a), a.state())
    for t in (a, b):
        t.set_hinges(hinges)
        t.set_hinge_targets(HW6[:3])
    a.set_hinge_trace(3, full=True)
    a.set_slider_trace(4, full=True)
    before, hbefore = _table(a, dev), _table(a, dev, hinge=True)
    got_q, got_om = _rollout(a, entry, dev, U, dt, iters)
    assert a.counter("rollout_launches") == T * _per_tick(entry, iters, hinges=True) + 3 + 4
    want_q, want_om, want, hwant = _loop(b, U, dt, iters, 4, True, before, hinge_rows=3, hinge_before=hbefore)
    got, hgot = _table(a, dev), _table(a, dev, hinge=True)
    assert got.tobytes() == want.tobytes(), SR.where(got, want)
    assert hgot.tobytes() == hwant.tobytes(), HR.where(hgot, hwant)
    assert got_q == want_q and got_om == want_om and not GR._same(a, b) and got[:, :, :8].any() and hgot[:, :, :8].any()
    # set_sliders behind a trace turns it off: the rollout is launch for launch what it is without the table
    a.set_hinge_trace(0)
    a.set_slider_trace(4)
    a.set_sliders(sliders)
    assert a.slider_trace_rows() == 0
    _rollout(a, entry, dev, U, dt, iters)
    assert a.counter("rollout_launches") == T * _per_tick(entry, iters, hinges=True)


RERUNS = [(e, d, (i + d) % 2 == 0, (6, 4)[(i + d) % 2], T) for i, e in enumerate(ENTRIES) for d in (False, True)] + [("rollout", True, True, 6, RC.T),
                                                                                                                   ("rollout_observe", False, False, 6, RC.T)]


@pytest.mark.parametrize("entry,dev,full,rows,ticks", RERUNS, ids=["%s-%s-%s-rows%d-T%d" % (e, "dev" if d else "host", "full" if f else "reading", r, t) for e, d, f, r, t in RERUNS])
def test_the_table_is_the_defining_loops_also_when_ticks_are_undone_and_run_again(ctx, entry, dev, full, rows, ticks):
    """cons_per_body = 1 - A's worlds outgrow their share in mid-call, so A's ticks are undone and run again while B never retries: a row
    written from the wrong pass, or the impulses of another tick's solve beside a reading, show.  T = 4: the last tick is run again;
    T = 6: ticks in the middle are, and later ticks of the earlier pass skip the undone world"""
    a, b, scs, u, planted, sliders = _twins(ctx, 1)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    assert RC.T == 6
    U = RC.controls(u, planted, ticks=ticks)
    a.set_slider_trace(rows, full=full)
    before = _table(a, dev)
    retries = a.counter("capacity_retries")
    got_q, got_om = _rollout(a, entry, dev, U, dt, iters)
    launches = a.counter("rollout_launches")
    assert a.counter("capacity_retries") > retries and launches > ticks * _per_tick(entry, iters) + min(ticks, rows)      # the re-run path was really taken
    want_q, want_om, want, _ = _loop(b, U, dt, iters, rows, full, before)
    assert b.counter("capacity_retries") == 0
    got = _table(a, dev)
    reach = min(ticks, rows)
    assert got.tobytes() == want.tobytes(), [(t, SR.where(got[t], want[t])) for t in range(reach) if got[t].tobytes() != want[t].tobytes()]
    assert got_q == want_q and got_om == want_om and not GR._same(a, b)
    assert not got[reach:].any() and got[:reach, :, :8].any()


# ---- a use case ---------------------------------------------------------------------------------------------------------------------------------
def test_a_policy_feels_the_limited_lift_through_the_trace(ctx):
    """tests/batch_slider_cases.py's lift - a body on a vertical slider to the world under gravity, limited to [-0.3, 0.4], a second body
    welded to it - through 64 ticks of a rollout that traces x, q, v and omega and fills the readings table in the full format: the traced
    d and rate equal lift_trace of the traced state rows within the derived bounds; `side` of the lift is +1 on exactly the ticks whose
    float64 d is above hi and 0 elsewhere - a tick whose d is within the d bound of a limit is left out, at most 2 of 64 -; `side` of the
    weld is 2 on every row; and the limit's impulse al[t] is 0 wherever the reading of the state tick t's solve set up from - row t - 1,
    row -1 being a read taken before the call - says the row is off."""
    import mgf_amd
    sc = LC.lift_scene()
    dt = float(sc["dt"])
    b = mgf_amd.WorldBatch.from_scenes(ctx, [sc], own_terrain=True)
    rig = LC.lift_rig(b.state(), True)
    b.set_sliders(rig)
    ticks = LC.LIFT_TICKS
    b.set_slider_trace(ticks, full=True)
    first = b.read_sliders()
    tr = b.rollout(ticks, dt, LC.LIFT_ITERS, trace=("x", "q", "v", "omega"))
    table = b.slider_trace()
    assert table.shape == (ticks, 2) and ticks == 64 and b.counter("sliders_skipped") == 0
    want_d, want_rate, gap, tilt = LC.lift_trace(rig, tr["x"], tr["q"], tr["v"], tr["omega"])
    bd, br = np.zeros(ticks), np.zeros(ticks)
    for t in range(ticks):
        row = {"x": tr["x"][t], "delta": np.zeros_like(tr["x"][t]), "q": tr["q"][t], "v": tr["v"][t], "omega": tr["omega"][t]}
        d_, o_, e_, r_ = SR.bounds(rig[:1], row, [2])
        bd[t], br[t] = d_[0], r_[0]
    d, rate = table["d"][:, 0].astype(np.float64), table["rate"][:, 0].astype(np.float64)
    print("the lift: largest |d - host d| %.3g (share of its bound %.3g), |rate - host rate| %.3g (share %.3g); d bound at most %.3g"
          % (np.abs(d - want_d).max(), (np.abs(d - want_d) / bd).max(), np.abs(rate - want_rate).max(), (np.abs(rate - want_rate) / br).max(), bd.max()))
    assert np.all(np.abs(d - want_d) <= bd) and np.all(np.abs(rate - want_rate) <= br)
    lo, hi = LC.LIFT_LIMIT
    near = np.minimum(np.abs(want_d - lo), np.abs(want_d - hi)) <= bd
    print("ticks within the bound of a limit:", int(near.sum()), "; the nearest is", float(np.minimum(np.abs(want_d - lo), np.abs(want_d - hi)).min()), "from it; above hi",
          int((want_d > hi).sum()), "below lo", int((want_d < lo).sum()))
    assert int(near.sum()) <= 2
    side = table["side"][:, 0]
    expect = np.where(want_d > hi, 1.0, np.where(want_d < lo, -1.0, 0.0))
    assert np.array_equal(side[~near], expect[~near]), np.flatnonzero(side != expect)
    assert np.any(want_d > hi) and np.any((want_d >= lo) & (want_d <= hi)) and not np.any(want_d < lo)       # the limit is met, and only hi
    assert np.all(table["side"][:, 1] == 2.0)                                    # the weld
    # the limit's impulse beside the reading: it acts in the tick after a reading that says so, never behind one that says the row is off
    assert first["side"][0] == 0.0 and first["side"][1] == 2.0
    al = table["al"][:, 0]
    prev = np.concatenate([first["side"][:1], side[:-1]])
    assert not al[prev == 0].any() and np.all(al[prev > 0] <= 0) and np.any(al < 0)
    assert not table["am"].any()                                                 # no motor here
    print("off-axis gap at most %.3g, frame error at most %.3g over the rollout" % (np.abs(table["off"]).max(), np.abs(table["e"]).max()))
