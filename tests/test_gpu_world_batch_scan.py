"""The sensor trace of a rollout (mgf_batch_rollout_observe / _rollout_observe_dev; WorldBatch.rollout_observe / .rollout_observe_dev)
against its definition, on twin batches as in tests/test_gpu_world_batch_trace.py: A takes ONE rollout_observe_dev, B the loop
[apply_springs_dev(dt)] | actuate_dev(u[t]) | step(1) | gather_state(row t) | [read_touches_dev(row t)] | cast_sensors_dev(kinds, row t)
the header defines it by, and the sensor rows, the touch rows, the state traces, the stats rows and everything a caller can read of the
batch are compared by bytes.  Every output buffer starts as 0x5A bytes, so an entry that is not written shows.  The test that carries the
weight is the second: A's worlds start with cons_per_body = 1 and outgrow their share in the MIDDLE of the rollout - ticks are undone and
run again, and the cast in the train is not gated - while B never retries.  T is RC.T or XC.T ticks."""
import numpy as np
import pytest

from tests import batch_actuator_cases as AC
from tests import batch_rollout_cases as RC
from tests import batch_scan_cases as YC
from tests import batch_sensor_cases as SC
from tests import batch_trace_cases as XC
from tests import test_gpu_world_batch_rollout as GR
from tests import test_gpu_world_batch_trace as GT

pytestmark = pytest.mark.gpu
IMPULSE, FORCE = AC.IMPULSE, AC.FORCE
FILL = 0x5A5A5A5A
ALL, BODIES, TERRAIN, OBSTACLES = 7, 1, 2, 4


@pytest.fixture(scope="module")
def ctx():
    import mgf_amd
    c = mgf_amd.Context(0)
    yield c
    c.close()


def _sensor_buffer(ticks, n, depth=False):
    import torch
    return torch.full((ticks, n) if depth else (ticks, n, 7), FILL, dtype=torch.int32, device="cuda")


def _hit_rows(words):
    from mgf_amd import _capi
    w = np.ascontiguousarray(words.cpu().numpy())
    return w.view(_capi.RAY_HIT_DTYPE).reshape(w.shape[0], w.shape[1])


def _observe(a, U, dt, iters, mode, body, kinds=ALL, depth=False, touches=None, names=("x", "q", "v", "omega"), ticks=None, sensors=True):
    """A's side: one rollout_observe_dev; touches: None, "full" or "short".  Returns (traces as bytes by name, the sensor rows - records,
    or float32 depths -, the touch rows or None, stats bytes)"""
    import torch
    ticks = (U if isinstance(U, int) else len(U)) if ticks is None else ticks
    n_act = a.actuator_count()
    m = len(a) if body is None else len(body)
    out = GR._buffers(ticks, m, names)
    rows = _sensor_buffer(ticks, a.sensor_count(), depth) if sensors else None
    tb = None if touches is None else GT._touch_buffer(ticks, a.touch_count(), touches == "short")
    ud = GR._dev(U) if n_act else ticks
    bd = None if body is None else GR._dev(body, np.int32)
    GR._sync()
    st = a.rollout_observe_dev(ud, dt, iters, mode, body=bd, touches=tb, short=touches == "short",
                               sensors=None if rows is None else rows.view(torch.float32) if depth else rows, depth=depth, kinds=kinds, **out)
    GR._sync()
    seen = None if rows is None else np.ascontiguousarray(rows.cpu().numpy()).view(np.float32) if depth else _hit_rows(rows)
    return ({k: out[k].cpu().numpy().tobytes() for k in out}, seen, None if tb is None else GT._rows(tb, touches == "short"), bytes(st))


def _loop(b, U, dt, iters, mode, body, kinds=ALL, touches=False, names=("x", "q", "v", "omega"), ticks=None):
    """B's side: the defining loop, call by call"""
    ticks = len(U) if ticks is None else ticks
    n_act = b.actuator_count()
    m = len(b) if body is None else len(body)
    out = GR._buffers(ticks, m, names)
    rows = _sensor_buffer(ticks, b.sensor_count())
    tb = GT._touch_buffer(ticks, b.touch_count()) if touches else None
    ud = GR._dev(U) if n_act else None
    bd = None if body is None else GR._dev(body, np.int32)
    GR._sync()
    stats = b""
    for t in range(ticks):
        if b.spring_count():
            b.apply_springs_dev(dt)
        if n_act:
            b.actuate_dev(ud[t], mode)
        stats += bytes(b.step(dt, iters, 1))
        if m and out:
            b.gather_state(bd, n=m, **{k: out[k][t] for k in out})
        if touches:
            b.read_touches_dev(tb[t])
        b.cast_sensors_dev(rows[t], kinds=kinds)
    GR._sync()
    return {k: out[k].cpu().numpy().tobytes() for k in out}, _hit_rows(rows), None if tb is None else GT._rows(tb), stats


def _differ(got, want):
    bad = [(t, i) for t in range(got.shape[0]) for i in range(got.shape[1]) if got[t, i].tobytes() != want[t, i].tobytes()]
    return len(bad), bad[:8]


def _cast(b, kinds):
    import torch
    out = torch.full((b.sensor_count(), 7), FILL, dtype=torch.int32, device="cuda")
    GR._sync()
    b.cast_sensors_dev(out, kinds=kinds)
    GR._sync()
    return _hit_rows(out[None])[0]


def _turned(ctx, scs, lay, count, own_terrain=True):
    """`count` batches of the scenes whose sensor bodies have turned for SC.TICKS ticks, the rig aimed from that state and set"""
    import mgf_amd
    out = []
    for _ in range(count):
        b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=own_terrain)
        key = np.unique(lay["world"].astype(np.int64) * 4096 + lay["body"])
        w, bd = (key // 4096).astype(np.int32), (key % 4096).astype(np.int32)
        om = np.random.default_rng(5).uniform(-9.0, 9.0, (len(w), 3)).astype(np.float32)
        b.set_velocities(w, bd, b.get(w, bd)["linear"], om)
        b.step(float(scs[0]["dt"]), scs[0]["iters"], SC.TICKS)
        out.append(b)
    rig = SC.aimed_rig(lay, scs, out[0].state(), GR._lengths(out[0]))
    for b in out:
        b.set_sensors(rig)
    assert not GR._same(out[0], out[-1])
    return out, rig


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [ALL, BODIES, TERRAIN])
def test_a_rollout_with_a_mixed_rig_is_the_loop_that_ends_in_cast_sensors(ctx, kinds):
    """SC.twin_scenes() over their own terrains: no sensor on world 0, one on the world of one body, 257 on the world of 300 (two work
    items) in one shuffled order, with and without IGNORE_SELF, one without a direction, dt = inf on most.  A: HIT rows, C: DEPTH rows,
    B: the loop."""
    scs = SC.twin_scenes()
    lay = SC.twin_layout(scs)
    (a, b, c), rig = _turned(ctx, scs, lay, 3)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    T = RC.T
    assert set(rig["flags"].tolist()) == {0, SC.IGNORE_SELF} and np.any(np.all(rig["d"] == 0, axis=1)) and np.any(np.isinf(rig["dt"])) and np.any(np.isfinite(rig["dt"]))
    assert np.bincount(rig["world"], minlength=3).tolist() == [0, 1, 257] and np.any(np.diff(rig["world"]) < 0)
    got, rows, _, got_stats = _observe(a, T, dt, iters, IMPULSE, None, kinds=kinds)
    want, full, _, want_stats = _loop(b, None, dt, iters, IMPULSE, None, kinds=kinds, ticks=T)
    assert rows.tobytes() == full.tobytes(), _differ(rows, full)
    assert not np.any(rows.view(np.uint32) == FILL)                                   # every entry was written
    for k, _ in GR.TRACES:
        assert got[k] == want[k], k
    assert got_stats == want_stats and not GR._same(a, b), GR._same(a, b)
    assert a.counter("capacity_retries") == 0 == b.counter("capacity_retries")
    # the rows are not trivial: they meet what the mask allows, and change from tick to tick
    allowed = {ALL: {-1, 0, 1, 2}, BODIES: {-1, 0}, TERRAIN: {-1, 1}}[kinds]
    assert set(full["kind"].ravel().tolist()) == allowed, sorted(set(full["kind"].ravel().tolist()))
    assert all(full[t].tobytes() != full[t + 1].tobytes() for t in range(T - 1))
    zero = np.all(rig["d"] == 0, axis=1)
    assert np.all(full["kind"][:, zero] == -1)
    # the depth rows: the hit's t, the sensor's dt where nothing is hit - bit for bit, inf among them
    got_c, depth, _, stats_c = _observe(c, T, dt, iters, IMPULSE, None, kinds=kinds, depth=True)
    want_depth = YC.depth_of(full, rig)
    assert depth.shape == (T, len(rig)) and depth.tobytes() == want_depth.tobytes(), np.argwhere(depth.view(np.uint32) != want_depth.view(np.uint32))[:8]
    assert np.any(np.isinf(depth)) and np.any(depth[full["kind"] == -1] == 1.0)
    assert got_c == want and stats_c == want_stats and not GR._same(c, b)
    # the cast behind the call: the gather behind the step still works, and the scratch does not leak
    for t in (a, c, b):
        assert _cast(t, kinds).tobytes() == full[T - 1].tobytes()
    assert _cast(a, ALL).tobytes() == _cast(b, ALL).tobytes()
    assert not GR._same(a, b)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [False, True])
def test_ticks_that_are_undone_and_run_again_in_mid_rollout_leave_every_row_the_loops(ctx, depth):
    """A's worlds start with cons_per_body = 1: LATE_A outgrows its share at its tick of first contact, LATE_B a tick later, so the call
    makes several passes.  In a pass that runs a tick again the cast is launched for EVERY world - the rows of the worlds that are not at
    that tick must not be written from it: SPARSE has finished the call, and a world that sits undone has its x and q put back but not
    the packed bodies the cast stages from.  B never retries.  tests/test_world_batch_scan_host.py holds the rig to the oracle: the rows
    of both late worlds differ between consecutive ticks, so a row written from the wrong tick shows.  (Run once on a build with
    -DMGF_SCAN_GATE=0, the rows' gate compiled to `true`: this test failed in both formats, 132 entries with wrong bytes, the first in
    tick 2's row; no other test was run on that build.)"""
    (a, b), scs, rig, u, planted = GR._late_twins(ctx, 2)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    T = XC.T
    srig = YC.late_sensor_rig()
    assert int(np.sum(srig["world"] == RC.LATE_A)) > 256                               # one world, two work items
    for t in (a, b):
        t.set_sensors(srig)
    U = RC.controls(u, planted, ticks=T)
    body, outside = RC.traced(len(a), count=30)
    got, rows, _, got_stats = _observe(a, U, dt, iters, IMPULSE, body, depth=depth)
    want, full, _, want_stats = _loop(b, U, dt, iters, IMPULSE, body)
    assert a.counter("capacity_retries") > 0 and b.counter("capacity_retries") == 0
    want_rows = YC.depth_of(full, srig) if depth else full
    from mgf_amd import _capi
    K = a.n_worlds
    st = (_capi.StepStats * (T * K)).from_buffer_copy(want_stats)
    cons = np.array([[st[t * K + k].n_constraints for k in range(K)] for t in range(T)])
    print("retries:", a.counter("capacity_retries"), "constraints per tick and world:", cons.tolist())
    assert rows.tobytes() == want_rows.tobytes(), _differ(rows, want_rows)
    assert not np.any(rows.view(np.uint32) == FILL)                                   # every entry was written
    for k, _ in GR.TRACES:
        assert got[k] == want[k], k
    assert got_stats == want_stats
    assert not GR._same(a, b), GR._same(a, b)
    # the worlds that re-ran: their rows differ between consecutive ticks at and behind the tick that outgrew the share
    for k in (RC.LATE_A, RC.LATE_B):
        rerun = next(t for t in range(T) if cons[t, k] > RC.share(a.world_len(k)))
        assert RC.FIRST_CONTACT <= rerun < T - 1, (k, cons[:, k].tolist())
        mine = want_rows[:, srig["world"] == k]
        for t in range(rerun - 1, T - 1):
            assert mine[t].tobytes() != mine[t + 1].tobytes(), (k, t)
    import mgf_amd
    per_tick = mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK + mgf_amd.BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK
    assert a.counter("rollout_launches") > T * per_tick                               # the passes that ran ticks again launched again
    assert a.counter("rollout_launches") % per_tick == 0                               # ... the trace with them, twice a tick a pass


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [ALL, BODIES | TERRAIN, OBSTACLES])
def test_the_obstacles_of_a_sensors_world_enter_its_row(ctx, kinds):
    scs = YC.obstacle_pair()
    lay = YC.obstacle_layout(scs)
    (a, b, c), rig = _turned(ctx, scs, lay, 3)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    T = RC.T
    got, rows, _, got_stats = _observe(a, T, dt, iters, IMPULSE, None, kinds=kinds)
    want, full, _, want_stats = _loop(b, None, dt, iters, IMPULSE, None, kinds=kinds, ticks=T)
    assert rows.tobytes() == full.tobytes(), _differ(rows, full)
    assert got == want and got_stats == want_stats and not GR._same(a, b)
    _, depth, _, _ = _observe(c, T, dt, iters, IMPULSE, None, kinds=kinds, depth=True)
    assert depth.tobytes() == YC.depth_of(full, rig).tobytes()
    hit = full["kind"] == YC.HIT_OBSTACLE
    if kinds & OBSTACLES:
        assert np.any(hit) and not np.any(hit[:, rig["world"] == 1])                   # the world without obstacles meets none
        # the obstacle pass changes an entry the body pass and the terrain walk alone would give: the same moment without the bit
        last = _cast(b, kinds & ~OBSTACLES) if kinds & ~OBSTACLES else None
        if last is not None:
            changed = hit[T - 1] & (last["kind"] != YC.HIT_NONE)
            assert np.any(changed) and np.all(full[T - 1]["t"][changed] <= last["t"][changed])
            assert full[T - 1][~hit[T - 1]].tobytes() == last[~hit[T - 1]].tobytes()
    else:
        assert not np.any(hit)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_springs_actuators_in_force_mode_a_touch_trace_and_a_sensor_trace_in_one_call(ctx):
    from tests import batch_spring_cases as SP
    (a, b, c), scs, rig, u, planted = GR._late_twins(ctx, 3)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    T = XC.T
    springs, s_planted = SP.late_springs(GR._lengths(a))
    touch_rig, srig = XC.late_touch_rig(), YC.late_sensor_rig()
    for t in (a, b, c):
        t.set_springs(springs)
        t.set_touches(touch_rig)
        t.set_sensors(srig)
    U = RC.controls(u, planted, ticks=T)
    body, outside = RC.traced(len(a), count=30)
    got, rows, touches, got_stats = _observe(a, U, dt, iters, FORCE, body, touches="short")
    want, full, full_touches, want_stats = _loop(b, U, dt, iters, FORCE, body, touches=True)
    assert a.counter("capacity_retries") > 0 and b.counter("capacity_retries") == 0 == c.counter("capacity_retries")
    assert rows.tobytes() == full.tobytes(), _differ(rows, full)
    assert touches.tobytes() == XC.short_of(full_touches).tobytes() and full_touches["n_contacts"].any()
    assert got == want and got_stats == want_stats and not GR._same(a, b)
    assert GT._skips(a) == GT._skips(b) and a.counter("springs_skipped") == T * len(s_planted)
    # ... and all but the sensor rows is rollout_touches_dev
    par, par_touches, par_stats = GT._rollout(c, U, dt, iters, FORCE, body, short=True)
    assert par == got and par_touches.tobytes() == touches.tobytes() and par_stats == got_stats and not GR._same(a, c)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_trace_adds_two_launches_a_tick_whatever_the_worlds_and_the_sensors(ctx):
    import mgf_amd
    assert mgf_amd.BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK == 2
    sc = RC.late_contact_scenes()[RC.SPARSE]
    dt, iters = float(sc["dt"]), sc["iters"]
    T = RC.T
    seen = []
    for K, n_act, m, n_sensor in ((3, 5, 4, 7), (12, 40, 60, 12 * 300)):
        b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K, own_terrain=True)
        rng = np.random.default_rng(K)
        b.set_actuators(rng.integers(0, K, n_act), rng.integers(0, 8, n_act), d=(0.0, 1.0, 0.0), gain=0.01)
        body = rng.integers(0, len(b), m).astype(np.int32)
        U = rng.uniform(-1, 1, (T, n_act)).astype(np.float32)
        # an empty sensor rig, and traces = None: the parents' counts exactly
        GR._rollout(b, U, dt, iters, IMPULSE, body)
        plain = b.counter("rollout_launches")
        assert plain == T * mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK
        _, rows, _, _ = _observe(b, U, dt, iters, IMPULSE, body)
        assert rows.shape == (T, 0) and b.counter("rollout_launches") == plain
        b.set_sensors(np.arange(n_sensor) % K, rng.integers(0, 8, n_sensor), p=(0.0, 0.0, 0.0), d=rng.normal(0, 1, (n_sensor, 3)))
        _observe(b, U, dt, iters, IMPULSE, body, sensors=False)
        assert b.counter("rollout_launches") == plain
        lib = mgf_amd.load_library()
        stats = (mgf_amd._capi.StepStats * (T * K))()
        ud, bd = GR._dev(U), GR._dev(body, np.int32)
        GR._sync()
        assert lib.mgf_batch_rollout_observe_dev(b._h, dt, iters, T, ud.data_ptr(), n_act, IMPULSE, bd.data_ptr(), m, None, None, None, None, None, stats) == 0
        assert b.counter("rollout_launches") == plain
        b.cast_sensors()
        query, drive = b.counter("query_launches"), b.counter("drive_launches")
        for depth in (False, True):
            _, rows, _, _ = _observe(b, U, dt, iters, IMPULSE, body, depth=depth)
            assert b.counter("capacity_retries") == 0                                # one pass: one host wait
            assert b.counter("rollout_launches") - plain == 2 * T
            assert b.counter("query_launches") == query and b.counter("drive_launches") == drive and b.counter("launches_per_tick") == 6
            assert not np.any(rows.view(np.uint32) == FILL)
        seen.append(b.counter("rollout_launches"))
        b.step(dt, iters, 1)
        assert b.counter("launches_per_tick") == 6
    assert seen[0] == seen[1]


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_host_form_is_the_device_form(ctx):
    from mgf_amd import _capi
    (a, b), scs, rig, u, planted = GR._late_twins(ctx, 2, cons_per_body_of_first=None)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    T = XC.T
    touch_rig, srig = XC.late_touch_rig(), YC.late_sensor_rig()
    for t in (a, b):
        t.set_touches(touch_rig)
        t.set_sensors(srig)
    U = RC.controls(u, planted, ticks=T)
    body, outside = RC.traced(len(a), count=30)
    inside = (body >= 0) & (body < len(a))
    got, rows, touches, got_stats = _observe(a, U, dt, iters, FORCE, body, touches="full")
    res = b.rollout_observe(U, dt, iters, FORCE, body=body, touches=True, sensors="hit")
    assert sorted(res) == ["omega", "q", "sensors", "stats", "touches", "v", "x"]
    assert res["sensors"].dtype == _capi.RAY_HIT_DTYPE and res["sensors"].shape == (T, len(srig)) and res["sensors"].tobytes() == rows.tobytes()
    assert res["touches"].tobytes() == touches.tobytes() and bytes(res["stats"]) == got_stats and not GR._same(a, b)
    for k, c in GR.TRACES:
        dev = np.frombuffer(got[k], np.float32).reshape(T, len(body), c)
        assert res[k][:, inside].tobytes() == dev[:, inside].tobytes() and not res[k][:, ~inside].any(), k
    # the depths alone: no state trace, no touch trace although the batch has a touch rig
    res = b.rollout_observe(U[:2], dt, iters, IMPULSE, trace=(), sensors="depth", kinds=BODIES)
    _, depth, _, got_stats = _observe(a, U[:2], dt, iters, IMPULSE, None, kinds=BODIES, depth=True, names=())
    assert sorted(res) == ["sensors", "stats"] and res["sensors"].dtype == np.float32 and res["sensors"].tobytes() == depth.tobytes()
    assert bytes(res["stats"]) == got_stats and not GR._same(a, b)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_that_need_the_handle_leave_the_batch_as_it_was(ctx):
    import mgf_amd
    import torch
    from mgf_amd import _capi
    from tests import batch_parts_cases as PC
    INV = _capi.ERR_INVALID
    (a, b), scs, rig, u, planted = GR._late_twins(ctx, 2, cons_per_body_of_first=None)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    srig = YC.late_sensor_rig()
    for t in (a, b):
        t.set_sensors(srig)
    lib = mgf_amd.load_library()
    n, ns, Tn = len(rig), len(srig), 3
    dev = torch.full((Tn * n + 7 * Tn * ns + 64,), FILL, dtype=torch.int32, device="cuda")
    GR._sync()
    up = dev.data_ptr()
    sp = up + 4 * Tn * n
    stats = (_capi.StepStats * (Tn * a.n_worlds))()
    host = np.full((Tn, ns, 7), FILL, np.int32)
    hu = np.zeros((Tn, n), np.float32)
    kept = GR._everything(a)

    def err():
        return lib.mgf_last_error().decode()

    def traces(sensor, n_sensor=ns, fmt=0, mask=ALL, reserved=0, word=0):
        tr = _capi.ROLLOUT_TRACES()
        tr.sensor, tr.n_sensor, tr.sensor_format, tr.sensor_mask = sensor, n_sensor, fmt, mask
        tr.reserved[word] = reserved
        return tr

    def dev_call(sensor=sp, n_act=n, **kw):
        tr = traces(sensor, **kw)
        return lib.mgf_batch_rollout_observe_dev(a._h, dt, iters, Tn, up, n_act, IMPULSE, None, 0, None, None, None, None, tr, stats)

    def host_call(sensor=host.ctypes.data, n_act=n, **kw):
        tr = traces(sensor, **kw)
        return lib.mgf_batch_rollout_observe(a._h, dt, iters, Tn, hu.ctypes.data, n_act, IMPULSE, None, 0, None, None, None, None, tr, stats)
    for call in (dev_call, host_call):
        for wrong in (ns - 1, ns + 1):
            assert call(n_sensor=wrong) == INV and "sensor_count" in err(), wrong
        for word in range(5):
            assert call(reserved=1 << word, word=word) == INV and "reserved" in err(), word
        for fmt in (2, -1):
            assert call(fmt=fmt) == INV and "sensor_format" in err(), fmt
        assert call(mask=8) == INV and call(n_sensor=-1) == INV and "n_sensor is negative" in err()
        assert call(n_act=n - 1, n_sensor=ns - 1) == INV and "actuator_count" in err()            # the actuators' length ahead of the sensors'
        assert call(fmt=2, reserved=1) == INV and "sensor_format" in err()                       # the format ahead of the reserved words
    assert dev_call(sensor=up) == INV and "overlaps" in err()                                     # the rows over the controls
    GR._sync()
    assert bool((dev == FILL).all().item()) and np.all(host == FILL)                              # nothing was written
    assert GR._everything(a) == kept and not GR._same(a, b)
    # a batch with a dumbbell: refused, option "part_queries" or not, although cast_sensors answers it under the option
    dsc = [PC.six_scenes()[PC.DUMBBELLS]]
    d, e = (mgf_amd.WorldBatch.from_scenes(ctx, dsc, own_terrain=True) for _ in range(2))
    for t in (d, e):
        t.step(float(dsc[0]["dt"]), dsc[0]["iters"], 2)
        t.set_sensors([0, 0], [0, 1], p=(0.0, 0.0, 0.0), d=(0.0, -1.0, 0.0))
    kept = GR._everything(d)
    for option in (0, 1):
        d.set_option("part_queries", option)
        e.set_option("part_queries", option)
        with pytest.raises(mgf_amd.MgfError, match="several components"):
            d.rollout_observe(2, float(dsc[0]["dt"]), dsc[0]["iters"], sensors="hit")
        with pytest.raises(mgf_amd.MgfError, match="several components"):
            d.rollout_observe_dev(2, float(dsc[0]["dt"]), dsc[0]["iters"], sensors=_sensor_buffer(2, 2))
        assert GR._everything(d) == kept and not GR._same(d, e)
    # ... and without a sensor trace it is answered, as by the parents
    res = d.rollout_observe(2, float(dsc[0]["dt"]), dsc[0]["iters"], trace=("x",))
    e.step(float(dsc[0]["dt"]), dsc[0]["iters"], 2)
    assert sorted(res) == ["stats", "x"] and not GR._same(d, e)
