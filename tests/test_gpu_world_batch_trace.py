"""The touch trace of a rollout (mgf_batch_rollout_touches / _rollout_touches_dev; WorldBatch.rollout_touches / .rollout_touches_dev)
against its definition, on twin batches as in tests/test_gpu_world_batch_rollout.py: A takes ONE rollout_touches_dev, B the loop
[apply_springs_dev(dt)] | actuate_dev(u[t]) | step(1) | gather_state(row t) | read_touches_dev(row t)  the header defines it by, and the
touch rows, the state traces, the stats rows, everything a caller can read of the batch and the skip counters are compared by bytes.
Every output buffer starts as 0x5A bytes, so a row that is not written shows.  The test that carries the weight is the second: A's worlds
start with cons_per_body = 1 and outgrow their share in the MIDDLE of the rollout - the lists move, ticks are undone and run again - while
B never retries.  The rigs are tests/batch_trace_cases.py's, T = 8 ticks."""
import numpy as np
import pytest

from tests import batch_actuator_cases as AC
from tests import batch_rollout_cases as RC
from tests import batch_touch_cases as TC
from tests import batch_trace_cases as XC
from tests import test_gpu_world_batch_rollout as GR

pytestmark = pytest.mark.gpu
IMPULSE, FORCE = AC.IMPULSE, AC.FORCE
T = XC.T
FILL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    import mgf_amd
    c = mgf_amd.Context(0)
    yield c
    c.close()


def _touch_buffer(ticks, n, short=False):
    import torch
    return torch.full((ticks, n, 4 if short else 16), FILL, dtype=torch.int32, device="cuda")


def _rows(words, short=False):
    """[T, n] records of the words a call wrote"""
    from mgf_amd import _capi
    w = np.ascontiguousarray(words.cpu().numpy())
    return w.view(_capi.TOUCH_SHORT_DTYPE if short else _capi.TOUCH_REPORT_DTYPE).reshape(w.shape[0], w.shape[1])


def _rollout(a, U, dt, iters, mode, body, short=False, names=("x", "q", "v", "omega"), ticks=None):
    """A's side: one rollout_touches_dev; returns (traces as bytes by name, the touch rows, stats bytes)"""
    ticks = len(U) if ticks is None else ticks
    n_act = a.actuator_count()
    m = len(a) if body is None else len(body)
    out = GR._buffers(ticks, m, names)
    touches = _touch_buffer(ticks, a.touch_count(), short)
    ud = GR._dev(U) if n_act else ticks
    bd = None if body is None else GR._dev(body, np.int32)
    GR._sync()
    st = a.rollout_touches_dev(ud, dt, iters, mode, body=bd, touches=touches, short=short, **out)
    GR._sync()
    return {k: out[k].cpu().numpy().tobytes() for k in out}, _rows(touches, short), bytes(st)


def _loop(b, U, dt, iters, mode, body, names=("x", "q", "v", "omega"), ticks=None, lists=False):
    """B's side: the defining loop, call by call; lists: also constraints(k) and q of every world behind every tick"""
    ticks = len(U) if ticks is None else ticks
    n_act = b.actuator_count()
    m = len(b) if body is None else len(body)
    out = GR._buffers(ticks, m, names)
    touches = _touch_buffer(ticks, b.touch_count())
    ud = GR._dev(U) if n_act else None
    bd = None if body is None else GR._dev(body, np.int32)
    GR._sync()
    stats, seen = b"", []
    for t in range(ticks):
        if b.spring_count():
            b.apply_springs_dev(dt)
        if n_act:
            b.actuate_dev(ud[t], mode)
        stats += bytes(b.step(dt, iters, 1))
        if m and out:
            b.gather_state(bd, n=m, **{k: out[k][t] for k in out})
        b.read_touches_dev(touches[t])
        if lists:
            seen.append(([b.constraints(k) for k in range(b.n_worlds)], [b.state(k)["q"] for k in range(b.n_worlds)]))
    GR._sync()
    return {k: out[k].cpu().numpy().tobytes() for k in out}, _rows(touches), stats, seen


def _differ(got, want):
    """(tick, sensor) of the rows that differ, the first few"""
    bad = [(t, i) for t in range(got.shape[0]) for i in range(got.shape[1]) if got[t, i].tobytes() != want[t, i].tobytes()]
    return bad[:8]


def _skips(t):
    return [t.counter(k) for k in ("actuators_skipped", "device_skipped", "springs_skipped")]


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [False, True])
@pytest.mark.parametrize("mode", [IMPULSE, FORCE])
def test_a_rollout_with_touches_is_the_loop_of_actuate_step_gather_and_read_touches(ctx, mode, short):
    (a, b), scs, rig, u, planted = GR._actuator_twins(ctx, 2)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    touch_rig = XC.actuator_touch_rig()
    for t in (a, b):
        t.set_touches(touch_rig)
    U = RC.controls(u, planted, ticks=T)
    body, outside = RC.traced(len(a))
    got, rows, got_stats = _rollout(a, U, dt, iters, mode, body, short=short)
    want, full, want_stats, seen = _loop(b, U, dt, iters, mode, body, lists=True)
    assert a.counter("capacity_retries") == 0 == b.counter("capacity_retries")
    want_rows = XC.short_of(full) if short else full
    assert rows.tobytes() == want_rows.tobytes(), _differ(rows, want_rows)
    for k, _ in GR.TRACES:
        assert got[k] == want[k], k
    assert got_stats == want_stats
    assert not GR._same(a, b), GR._same(a, b)
    assert _skips(a) == _skips(b) and a.counter("actuators_skipped") == T * len(planted)
    # the definition itself: the fold of B's own lists and rows q, tick by tick
    folded = XC.fold_ticks(touch_rig, [s[0] for s in seen], [s[1] for s in seen])
    assert full.tobytes() == folded.tobytes(), _differ(full, folded)
    # the rows are not trivial: every kind and both frames report contacts, and the rows change from tick to tick
    touched = full["n_contacts"].max(axis=0) > 0
    kinds = np.array([str(XC.kind(s)) for s in touch_rig])
    assert all(np.any(touched & (kinds == str(kd))) for kd in TC.KINDS) and all(np.any(touched & (touch_rig["flags"] == fr)) for fr in (0, 1))
    assert all(rows[t].tobytes() != rows[t + 1].tobytes() for t in range(T - 1))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [False, True])
def test_ticks_that_are_undone_and_run_again_in_mid_rollout_leave_every_row_the_loops(ctx, short):
    """A's worlds start with cons_per_body = 1: LATE_A outgrows its share at its tick of first contact, LATE_B a tick later, so the call
    makes several passes, batch_allot moves the constraint lists between them, and in the second pass LATE_B sits undone one tick ahead
    of the tick the pass starts from, while SPARSE has finished the call.  B never retries.  What this catches: touch arguments captured
    once ahead of the first pass - batch_allot swaps in a NEW list buffer and a NEW offsets table and frees the old ones, so the later
    passes would fold freed storage, and the rows of the ticks that are run again differ (by reading the code; never run); and a launch
    that does not obey the gate - SPARSE's rows of the re-run ticks are then written again from its LAST list (run once, on a scratch
    build whose kernel took `on = true`: this test failed in both formats, the first rows that differ tick 2's of world SPARSE, and of
    the others only the springs' test with cons_per_body = 1 failed, in the same way).  What it
    does NOT catch: a gate on `done` alone.  It differs from the kernel's for a world that sits undone one tick ahead (LATE_B in the
    second pass), and as the tick's kernels stand such a world's list, count and q are still tick t's: the row written again has the
    same bytes.  The second half of the condition is the record's, kept so that the trace does not lean on that."""
    (a, b), scs, rig, u, planted = GR._late_twins(ctx, 2)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    touch_rig = XC.late_touch_rig()
    assert int(np.sum(touch_rig["world"] == RC.LATE_A)) > 256                       # one world, two work items
    for t in (a, b):
        t.set_touches(touch_rig)
    U = RC.controls(u, planted, ticks=T)
    body, outside = RC.traced(len(a), count=30)
    got, rows, got_stats = _rollout(a, U, dt, iters, IMPULSE, body, short=short)
    want, full, want_stats, seen = _loop(b, U, dt, iters, IMPULSE, body, lists=True)
    assert a.counter("capacity_retries") > 0 and b.counter("capacity_retries") == 0
    want_rows = XC.short_of(full) if short else full
    print("retries:", a.counter("capacity_retries"), "records per tick and world:", [[len(c) for c in s[0]] for s in seen])
    assert rows.tobytes() == want_rows.tobytes(), _differ(rows, want_rows)
    words = rows.view(np.uint32)
    assert not np.any(words == FILL)                                                 # every entry was written
    for k, _ in GR.TRACES:
        assert got[k] == want[k], k
    assert got_stats == want_stats
    assert not GR._same(a, b), GR._same(a, b)
    assert _skips(a) == _skips(b)
    folded = XC.fold_ticks(touch_rig, [s[0] for s in seen], [s[1] for s in seen])
    assert full.tobytes() == folded.tobytes(), _differ(full, folded)
    # the re-runs happened where the contacts are, and the rows around them differ from tick to tick in both worlds of the pair
    for k in (RC.LATE_A, RC.LATE_B):
        counts = [len(s[0][k]) for s in seen]
        first = next(t for t in range(T) if counts[t])
        assert RC.FIRST_CONTACT <= first < T - 1 and max(counts) > RC.share(a.world_len(k)), (k, counts)
        mine = full[:, touch_rig["world"] == k]
        assert not mine["n_contacts"][:first].any() and mine["n_contacts"][first].any()
        assert len({mine[t].tobytes() for t in range(first, T)}) > 1, k
    import mgf_amd
    per_tick = mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK + mgf_amd.BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK
    assert a.counter("rollout_launches") > T * per_tick                               # the passes that ran ticks again launched again
    assert a.counter("rollout_launches") % per_tick == 0                               # ... the trace with them, once a tick a pass


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cons_per_body", [None, 1])
def test_with_a_spring_rig_the_loop_starts_with_apply_springs(ctx, cons_per_body):
    from tests import batch_spring_cases as SP
    (a, b), scs, rig, u, planted = GR._late_twins(ctx, 2, cons_per_body_of_first=cons_per_body)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    springs, s_planted = SP.late_springs(GR._lengths(a))
    touch_rig = XC.late_touch_rig()
    for t in (a, b):
        t.set_springs(springs)
        t.set_touches(touch_rig)
    U = RC.controls(u, planted, ticks=T)
    body, outside = RC.traced(len(a), count=30)
    got, rows, got_stats = _rollout(a, U, dt, iters, IMPULSE, body)
    want, full, want_stats, _ = _loop(b, U, dt, iters, IMPULSE, body)
    assert (a.counter("capacity_retries") > 0) == (cons_per_body == 1) and b.counter("capacity_retries") == 0
    assert rows.tobytes() == full.tobytes(), _differ(rows, full)
    assert got == want and got_stats == want_stats and not GR._same(a, b)
    assert _skips(a) == _skips(b) and a.counter("springs_skipped") == T * len(s_planted)
    assert full["n_contacts"].any()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_with_dumbbells_is_answered(ctx):
    import mgf_amd
    from tests import batch_parts_cases as PC
    dsc = [PC.six_scenes()[PC.DUMBBELLS]]
    dt, iters = float(dsc[0]["dt"]), dsc[0]["iters"]
    a, b = (mgf_amd.WorldBatch.from_scenes(ctx, dsc, own_terrain=True) for _ in range(2))
    for t in (a, b):
        t.step(dt, iters, TC.PARTS_TICK)                                             # the bodies lie on each other
    n = GR._lengths(a)[0]
    touch_rig = TC.layout(a.constraints(0), n, 0, spread=n)
    drig, du = AC.dumbbell_rig(n)
    for t in (a, b):
        t.set_actuators(drig)
        t.set_touches(touch_rig)
    U = RC.controls(du, [], ticks=T)
    body = np.int32([n - 1, 0, n - 1, 3])
    for short in (False, True):
        got, rows, got_stats = _rollout(a, U, dt, iters, IMPULSE, body, short=short)
        want, full, want_stats, _ = _loop(b, U, dt, iters, IMPULSE, body)
        want_rows = XC.short_of(full) if short else full
        assert rows.tobytes() == want_rows.tobytes(), _differ(rows, want_rows)
        assert got == want and got_stats == want_stats and not GR._same(a, b), short
        assert a.counter("launches_per_tick") == 7 == b.counter("launches_per_tick")
        assert a.counter("rollout_launches") == T * (mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK + mgf_amd.BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK)
        on_dumbbell = touch_rig["body"] == n - 1                                     # (the bodies of two parts come last)
        assert full["n_contacts"][:, on_dumbbell].any() and full["n_contacts"][:, ~on_dumbbell].any()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_degenerate_calls_and_refusals_that_need_the_handle(ctx):
    import mgf_amd
    import torch
    from mgf_amd import _capi
    INV = _capi.ERR_INVALID
    (a, b), scs, rig, u, planted = GR._late_twins(ctx, 2, cons_per_body_of_first=None)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    U = RC.controls(u, planted, ticks=T)
    body, outside = RC.traced(len(a), count=30)
    # an empty sensor rig, n_touch = 0: rollout_dev, in bytes and in launches
    got, rows, got_stats = _rollout(a, U, dt, iters, IMPULSE, body)
    want, want_stats = GR._rollout(b, U, dt, iters, IMPULSE, body)
    assert rows.shape == (T, 0) and got == want and got_stats == want_stats and not GR._same(a, b)
    assert a.counter("rollout_launches") == b.counter("rollout_launches") == T * mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK
    st = a.rollout_touches_dev(GR._dev(U), dt, iters, body=GR._dev(body, np.int32))    # touches=None
    assert bytes(st) == bytes(b.rollout_dev(GR._dev(U), dt, iters, body=GR._dev(body, np.int32))) and not GR._same(a, b)
    assert a.counter("rollout_launches") == b.counter("rollout_launches") > 0
    # with a rig: no ticks, nothing written
    touch_rig = XC.late_touch_rig()
    for t in (a, b):
        t.set_touches(touch_rig)
    n_touch = len(touch_rig)
    kept = GR._everything(a)
    touches = _touch_buffer(0, n_touch)
    assert len(a.rollout_touches_dev(GR._dev(U[:0]), dt, iters, touches=touches)) == 0 and GR._everything(a) == kept
    assert a.counter("rollout_launches") == 0
    # refusals: the batch, the rig and the buffers as they were
    lib = mgf_amd.load_library()
    n, m, Tn = len(rig), 5, 3
    words = Tn * n + m + 13 * Tn * m + 16 * Tn * n_touch
    dev = torch.full((words + 64,), FILL, dtype=torch.int32, device="cuda")
    GR._sync()
    up = dev.data_ptr()
    bp = up + 4 * Tn * n
    xp = bp + 4 * m
    qp, vp, op = xp + 12 * Tn * m, xp + 28 * Tn * m, xp + 40 * Tn * m
    tp = xp + 52 * Tn * m
    stats = (_capi.StepStats * (Tn * a.n_worlds))()
    host = np.full((Tn, n_touch, 16), FILL, np.int32)
    hu, hb, hx = np.zeros((Tn, n), np.float32), np.zeros(m, np.int32), np.full((Tn, m, 3), 7.0, np.float32)

    def err():
        return lib.mgf_last_error().decode()

    def dev_call(n_ticks=Tn, x=xp, touch=tp, n_touch=n_touch, fmt=_capi.ROLLOUT_TOUCH_FULL, n_act=n, mode=IMPULSE):
        return lib.mgf_batch_rollout_touches_dev(a._h, dt, iters, n_ticks, up, n_act, mode, bp, m, x, qp, vp, op, touch, n_touch, fmt, stats)

    def host_call(n_ticks=Tn, touch=host.ctypes.data, n_touch=n_touch, fmt=_capi.ROLLOUT_TOUCH_FULL, n_act=n, mode=IMPULSE, **_):
        return lib.mgf_batch_rollout_touches(a._h, dt, iters, n_ticks, hu.ctypes.data, n_act, mode, hb.ctypes.data, m, hx.ctypes.data, None, None, None,
                                             touch, n_touch, fmt, stats)
    for call in (dev_call, host_call):
        for wrong in (n_touch - 1, n_touch + 1, 0):
            assert call(n_touch=wrong) == INV and "touch_count" in err(), wrong
        for fmt in (2, -1, 64):
            assert call(fmt=fmt) == INV and "touch_format" in err(), fmt
        assert call(n_touch=-1) == INV and "n_touch is negative" in err()
        assert call(touch=None) == INV and "NULL argument: touch" in err()
        assert call(n_act=n - 1, n_touch=n_touch - 1) == INV and "actuator_count" in err()        # the actuators' length ahead of the sensors'
        assert call(mode=2, fmt=2) == INV and "mode" in err()                                    # the mode ahead of the format
    # the device form's own: the touch rows over another output or an input (all of it device memory)
    assert dev_call(touch=xp) == INV and "touch_dev" in err() and "overlaps" in err()
    assert dev_call(touch=tp - 4) == INV and "overlaps" in err()                     # over the end of omega
    assert dev_call(touch=up) == INV and "overlaps" in err()
    assert dev_call(x=tp + 64 * Tn * n_touch - 12 * Tn * m) == INV and "overlaps" in err()       # x over the end of the touch rows
    assert dev_call(touch=tp + 2) == INV and "aligned" in err()
    GR._sync()
    assert bool((dev == FILL).all().item()) and np.all(host == FILL) and np.all(hx == 7.0)      # nothing was written
    assert a.touch_count() == n_touch and GR._everything(a) == kept and not GR._same(a, b)
    # and the batch is as it was: the next call is the twin's loop (B ran two rollouts above, as A did)
    got, rows, got_stats = _rollout(a, U, dt, iters, IMPULSE, None)
    want, full, want_stats, _ = _loop(b, U, dt, iters, IMPULSE, None)
    assert rows.tobytes() == full.tobytes() and got == want and got_stats == want_stats and not GR._same(a, b)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_trace_adds_one_launch_a_tick_whatever_the_worlds_and_the_sensors(ctx):
    import mgf_amd
    assert mgf_amd.BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK == 1
    sc = RC.late_contact_scenes()[RC.SPARSE]
    dt, iters = float(sc["dt"]), sc["iters"]
    seen = []
    for K, n_act, m, n_touch in ((3, 5, 4, 7), (12, 40, 60, 12 * 300)):
        b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K, own_terrain=True)
        rng = np.random.default_rng(K)
        b.set_actuators(rng.integers(0, K, n_act), rng.integers(0, 8, n_act), d=(0.0, 1.0, 0.0), gain=0.01)
        b.set_touches(np.arange(n_touch) % K, rng.integers(0, 8, n_touch), other=mgf_amd.TOUCH_ANY)
        body = rng.integers(0, len(b), m).astype(np.int32)
        U = rng.uniform(-1, 1, (T, n_act)).astype(np.float32)
        # what the parents leave: the step nothing, rollout_dev its two a tick
        b.step(dt, iters, 2)
        assert b.counter("rollout_launches") == 0 and b.counter("launches_per_tick") == 6
        GR._rollout(b, U, dt, iters, IMPULSE, body)
        plain = b.counter("rollout_launches")
        assert plain == T * mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK
        b.read_touches()
        query = b.counter("query_launches")
        drive = b.counter("drive_launches")
        _, rows, _ = _rollout(b, U, dt, iters, IMPULSE, body)
        assert b.counter("capacity_retries") == 0                                    # one pass: one host wait
        assert b.counter("rollout_launches") == T * (plain // T + mgf_amd.BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK)
        assert b.counter("query_launches") == query and b.counter("drive_launches") == drive and b.counter("launches_per_tick") == 6
        assert not np.any(rows.view(np.uint32) == FILL)
        seen.append(b.counter("rollout_launches"))
        b.step(dt, iters, 1)
        assert b.counter("launches_per_tick") == 6
    assert seen[0] == seen[1]


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", [False, True])
def test_the_host_form_is_the_device_form(ctx, short):
    from mgf_amd import _capi
    (a, b), scs, rig, u, planted = GR._late_twins(ctx, 2, cons_per_body_of_first=None)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    touch_rig = XC.late_touch_rig()
    for t in (a, b):
        t.set_touches(touch_rig)
    U = RC.controls(u, planted, ticks=T)
    body, outside = RC.traced(len(a), count=30)
    inside = (body >= 0) & (body < len(a))
    got, rows, got_stats = _rollout(a, U, dt, iters, FORCE, body, short=short)
    res = b.rollout_touches(U, dt, iters, FORCE, body=body, short=short)
    assert sorted(res) == ["omega", "q", "stats", "touches", "v", "x"]
    assert res["touches"].dtype == (_capi.TOUCH_SHORT_DTYPE if short else _capi.TOUCH_REPORT_DTYPE) and res["touches"].shape == (T, len(touch_rig))
    assert res["touches"].tobytes() == rows.tobytes() and rows["n_contacts"].any()
    assert bytes(res["stats"]) == got_stats and not GR._same(a, b)
    for k, c in GR.TRACES:
        dev = np.frombuffer(got[k], np.float32).reshape(T, len(body), c)
        assert res[k][:, inside].tobytes() == dev[:, inside].tobytes() and not res[k][:, ~inside].any(), k
    # the touch rows alone, no state trace
    res = b.rollout_touches(U[:2], dt, iters, IMPULSE, trace=(), short=short)
    got, rows, got_stats = _rollout(a, U[:2], dt, iters, IMPULSE, None, short=short, names=())
    assert sorted(res) == ["stats", "touches"] and res["touches"].tobytes() == rows.tobytes() and bytes(res["stats"]) == got_stats and not GR._same(a, b)
