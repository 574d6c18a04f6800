"""The rollouts of a batch (mgf_batch_rollout / _rollout_dev; WorldBatch.rollout / .rollout_dev) against their definition, on twin
batches: A takes ONE rollout, B the loop  actuate_dev(u[t]) | step(1) | gather_state(row t)  the header defines it by, and everything a
caller can read is compared by bytes - state() and get() (the force and torque rows) of every body, constraints(k) of every world, the
traces against B's gathers tick by tick, the stats rows, "actuators_skipped", "device_skipped".  The test that carries the weight is
the second: A's worlds start with cons_per_body = 1 and outgrow their share in the MIDDLE of the rollout, so A's ticks are undone and
run again while B never retries - a control row applied twice or not at all, or a trace row written from the wrong tick, shows."""
import numpy as np
import pytest

from tests import batch_actuator_cases as AC
from tests import batch_drive_cases as DC
from tests import batch_rollout_cases as RC

pytestmark = pytest.mark.gpu
IMPULSE, FORCE = AC.IMPULSE, AC.FORCE
TRACES = (("x", 3), ("q", 4), ("v", 3), ("omega", 3))


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


def _everything(b):
    """what a caller can read of the batch: state() and get() of every body, the constraint list of every world - as bytes"""
    w, bd = _all(b)
    st = b.state()
    return [st[k].tobytes() for k in DC.STATE] + [b.get(w, bd).tobytes()] + [b.constraints(k).tobytes() for k in range(b.n_worlds)]


def _same(a, b):
    ea, eb = _everything(a), _everything(b)
    return [i for i in range(len(ea)) if ea[i] != eb[i]]


def _buffers(T, m, names=("x", "q", "v", "omega")):
    """trace buffers that start as 0x5A bytes: a row a call does not write shows, and is the same on both twins"""
    import torch
    return {k: torch.full((T, m, c), 0x5A5A5A5A, dtype=torch.int32, device="cuda").view(torch.float32) for k, c in TRACES if k in names}


def _dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _rollout(a, U, dt, iters, mode, body, names=("x", "q", "v", "omega"), T=None):
    """A's side: one rollout_dev; returns (traces as bytes by name, stats bytes)"""
    T = len(U) if T is None else T
    n_act = a.actuator_count()
    m = len(a) if body is None else len(body)
    out = _buffers(T, m, names)
    ud = _dev(U) if n_act else T
    bd = None if body is None else _dev(body, np.int32)
    _sync()
    st = a.rollout_dev(ud, dt, iters, mode, body=bd, **out)
    _sync()
    return {k: out[k].cpu().numpy().tobytes() for k in out}, bytes(st)


def _loop(b, U, dt, iters, mode, body, names=("x", "q", "v", "omega"), T=None):
    """B's side: the defining loop, call by call"""
    T = len(U) if T is None else T
    n_act = b.actuator_count()
    m = len(b) if body is None else len(body)
    out = _buffers(T, m, names)
    ud = _dev(U) if n_act else None
    bd = None if body is None else _dev(body, np.int32)
    _sync()
    stats = b""
    for t in range(T):
        if n_act:
            b.actuate_dev(ud[t], mode)
        stats += bytes(b.step(dt, iters, 1))
        if m and out:
            b.gather_state(bd, n=m, **{k: out[k][t] for k in out})
    _sync()
    return {k: out[k].cpu().numpy().tobytes() for k in out}, stats


def _actuator_twins(ctx, count, seed=7):
    """`count` batches of AC.actuator_scenes(), spun and ticked until the bodies have turned, the main rig set"""
    import mgf_amd
    scs = AC.actuator_scenes()
    out = []
    for _ in range(count):
        b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
        w, bd = _all(b)
        om = np.random.default_rng(seed).uniform(-9.0, 9.0, (len(w), 3)).astype(np.float32)
        b.set_velocities(w, bd, b.get(w, bd)["linear"], om)
        b.step(float(scs[0]["dt"]), scs[0]["iters"], AC.TICKS)
        b.add_bodies(AC.LATE_WORLD, *AC.late_bodies(scs[AC.LATE_WORLD]))
        out.append(b)
    rig, u, planted = AC.main_rig(_lengths(out[0]))
    for b in out:
        b.set_actuators(rig)
    assert not _same(out[0], out[-1])
    return out, scs, rig, u, planted


def _late_twins(ctx, count, cons_per_body_of_first=1):
    """batches of RC.late_contact_scenes() with the late rig; the first starts with cons_per_body = 1"""
    import mgf_amd
    scs = RC.late_contact_scenes()
    out = []
    for i in range(count):
        b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
        if i == 0 and cons_per_body_of_first is not None:
            b.set_option("cons_per_body", cons_per_body_of_first)
        out.append(b)
    rig, u, planted = RC.late_rig(_lengths(out[0]))
    for b in out:
        b.set_actuators(rig)
    return out, scs, rig, u, planted


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [IMPULSE, FORCE])
def test_a_rollout_is_the_loop_of_actuate_step_and_gather(ctx, mode):
    (a, b), scs, rig, u, planted = _actuator_twins(ctx, 2)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    assert 400 <= len(rig) <= 500 and len(planted) == 3
    U = RC.controls(u, planted)
    body, outside = RC.traced(len(a))
    assert outside == 2 and len(set(body.tolist())) == len(body) - 1
    skipped0 = [t.counter("device_skipped") for t in (a, b)]
    got, got_stats = _rollout(a, U, dt, iters, mode, body)
    want, want_stats = _loop(b, U, dt, iters, mode, body)
    for k, _ in TRACES:
        assert got[k] == want[k], k
    assert got["v"] != bytes(len(got["v"]))
    assert got_stats == want_stats
    assert not _same(a, b), _same(a, b)
    assert a.counter("actuators_skipped") == b.counter("actuators_skipped") == RC.T * len(planted)
    assert [t.counter("device_skipped") - s for t, s in zip((a, b), skipped0)] == [outside * RC.T] * 2
    # the rows differ from tick to tick
    rows = np.frombuffer(got["v"], np.float32).reshape(RC.T, len(body), 3)
    assert all(rows[t].tobytes() != rows[t + 1].tobytes() for t in range(RC.T - 1))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [IMPULSE, FORCE])
def test_ticks_that_are_undone_and_run_again_in_mid_rollout_change_nothing(ctx, mode):
    (a, b), scs, rig, u, planted = _late_twins(ctx, 2)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    K = a.n_worlds
    U = RC.controls(u, planted)
    body, outside = RC.traced(len(a), count=30)
    skipped0 = [t.counter("device_skipped") for t in (a, b)]
    got, got_stats = _rollout(a, U, dt, iters, mode, body)
    want, want_stats = _loop(b, U, dt, iters, mode, body)
    assert a.counter("capacity_retries") > 0 and b.counter("capacity_retries") == 0
    import mgf_amd
    from mgf_amd import _capi
    st = (_capi.StepStats * (RC.T * K)).from_buffer_copy(want_stats)
    cons = np.array([[st[t * K + k].n_constraints for k in range(K)] for t in range(RC.T)])
    print("constraints per tick and world:", cons.tolist(), "retries:", a.counter("capacity_retries"))
    for k in (RC.LATE_A, RC.LATE_B):
        first = int(np.flatnonzero(cons[:, k])[0])
        assert first >= RC.FIRST_CONTACT, (k, cons[:, k].tolist())
        assert cons[:, k].max() > RC.share(a.world_len(k)), (k, cons[:, k].tolist())        # the re-run happened where the contacts are
    assert cons[:, RC.SPARSE].max() <= RC.share(a.world_len(RC.SPARSE))
    for k, _ in TRACES:
        row = len(got[k]) // RC.T
        assert got[k] == want[k], (k, "ticks whose rows differ:", [t for t in range(RC.T) if got[k][t * row:(t + 1) * row] != want[k][t * row:(t + 1) * row]])
    assert got_stats == want_stats
    assert not _same(a, b), _same(a, b)
    assert a.counter("actuators_skipped") == b.counter("actuators_skipped") == RC.T * len(planted)
    assert [t.counter("device_skipped") - s for t, s in zip((a, b), skipped0)] == [outside * RC.T] * 2
    assert a.counter("rollout_launches") > RC.T * mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK   # the passes that ran ticks again launched again


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_no_actuators_no_trace_one_output_and_every_body(ctx):
    import mgf_amd
    scs = RC.late_contact_scenes()
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    a, b = (mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True) for _ in range(2))
    U = np.zeros((RC.T, 0), np.float32)
    # an empty rig with a trace of every body (body=None): step(1) + gather
    got, got_stats = _rollout(a, U, dt, iters, IMPULSE, None)
    want, want_stats = _loop(b, U, dt, iters, IMPULSE, None)
    assert got == want and got_stats == want_stats and not _same(a, b)
    assert a.counter("rollout_launches") == RC.T                                # the record launch alone
    # an empty rig and nothing traced: step(dt, iters, T), stats and all
    import torch
    st = a.rollout_dev(RC.T, dt, iters, body=torch.zeros(0, dtype=torch.int32, device="cuda"))
    want_st = b.step(dt, iters, RC.T)
    assert bytes(st) == bytes(want_st) and not _same(a, b) and a.counter("rollout_launches") == 0
    # bodies named but no output given: the ticks alone
    body, _ = RC.traced(len(a), count=10)
    skipped0 = a.counter("device_skipped")
    st = a.rollout_dev(2, dt, iters, body=_dev(body, np.int32))
    assert bytes(st) == bytes(b.step(dt, iters, 2)) and not _same(a, b) and a.counter("rollout_launches") == 0
    assert a.counter("device_skipped") == skipped0                              # as the gather without an output: nothing is counted
    # one output array
    for name in ("q", "omega"):
        got, got_stats = _rollout(a, U[:3], dt, iters, IMPULSE, body, names=(name,))
        want, want_stats = _loop(b, U[:3], dt, iters, IMPULSE, body, names=(name,))
        assert list(got) == [name] and got == want and got_stats == want_stats and not _same(a, b), name
    # no ticks: nothing happens
    kept = _everything(a)
    assert len(a.rollout_dev(0, dt, iters)) == 0 and _everything(a) == kept and a.counter("rollout_launches") == 0


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_host_form_is_the_device_form(ctx):
    (a, b), scs, rig, u, planted = _late_twins(ctx, 2, cons_per_body_of_first=None)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    U = RC.controls(u, planted)
    body, outside = RC.traced(len(a), count=30)
    inside = (body >= 0) & (body < len(a))
    got, got_stats = _rollout(a, U, dt, iters, FORCE, body)
    res = b.rollout(U, dt, iters, FORCE, body=body)
    assert sorted(res) == ["omega", "q", "stats", "v", "x"]
    assert bytes(res["stats"]) == got_stats and not _same(a, b)
    for k, c in TRACES:
        dev = np.frombuffer(got[k], np.float32).reshape(RC.T, len(body), c)
        assert res[k].shape == dev.shape and res[k][:, inside].tobytes() == dev[:, inside].tobytes(), k
        assert not res[k][:, ~inside].any()                                     # the host form's rows of an index outside the batch: zeros
    assert a.counter("actuators_skipped") == b.counter("actuators_skipped") == RC.T * len(planted)
    assert a.counter("device_skipped") == b.counter("device_skipped") == outside * RC.T
    # a subset of the traces, every body
    res = b.rollout(U[:2], dt, iters, IMPULSE, trace=("v",))
    got, got_stats = _rollout(a, U[:2], dt, iters, IMPULSE, None, names=("v",))
    assert sorted(res) == ["stats", "v"] and res["v"].tobytes() == got["v"] and bytes(res["stats"]) == got_stats and not _same(a, b)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_with_dumbbells_is_answered(ctx):
    import mgf_amd
    from tests import batch_parts_cases as PC
    dsc = [PC.six_scenes()[PC.DUMBBELLS]]
    dt, iters = float(dsc[0]["dt"]), dsc[0]["iters"]
    a, b = (mgf_amd.WorldBatch.from_scenes(ctx, dsc, own_terrain=True) for _ in range(2))
    for t in (a, b):
        t.step(dt, iters, 4)
    n = _lengths(a)[0]
    drig, du = AC.dumbbell_rig(n)
    for t in (a, b):
        t.set_actuators(drig)
    U = RC.controls(du, [])
    body = np.int32([n - 1, 0, n - 1, 3])
    for mode in (IMPULSE, FORCE):
        got, got_stats = _rollout(a, U, dt, iters, mode, body)
        want, want_stats = _loop(b, U, dt, iters, mode, body)
        assert got == want and got_stats == want_stats and not _same(a, b), mode
        assert a.counter("launches_per_tick") == 7 == b.counter("launches_per_tick")
        assert a.counter("rollout_launches") == RC.T * mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_launches_of_a_rollout_depend_on_neither_the_worlds_nor_the_records(ctx):
    import mgf_amd
    assert mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK == 2
    sc = RC.late_contact_scenes()[RC.SPARSE]
    dt, iters = float(sc["dt"]), sc["iters"]
    seen = []
    for K, n_act, m in ((1, 1, 1), (300, 900, 1200)):
        b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K, own_terrain=True)
        rng = np.random.default_rng(K)
        b.set_actuators(rng.integers(0, K, n_act), rng.integers(0, 8, n_act), d=(0.0, 1.0, 0.0), gain=0.01)
        b.gather_state(None, x=_buffers(1, len(b), ("x",))["x"][0])
        drive = b.counter("drive_launches")
        assert drive == 1
        body = rng.integers(0, len(b), m).astype(np.int32)
        _rollout(b, rng.uniform(-1, 1, (RC.T, n_act)).astype(np.float32), dt, iters, IMPULSE, body)
        assert b.counter("capacity_retries") == 0
        seen.append(b.counter("rollout_launches"))
        assert b.counter("launches_per_tick") == 6 and b.counter("drive_launches") == drive
    assert seen == [RC.T * mgf_amd.BATCH_ROLLOUT_LAUNCHES_PER_TICK] * 2


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_rigs_and_readers_report_the_last_tick_and_the_batch_goes_on_as_the_loops(ctx):
    (a, b), scs, rig, u, planted = _late_twins(ctx, 2)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    lens = _lengths(a)
    rng = np.random.default_rng(5)
    w = np.repeat(np.arange(3, dtype=np.int32), 12)
    bd = np.concatenate([rng.integers(0, lens[k], 12) for k in range(3)]).astype(np.int32)
    d = rng.normal(0, 1, (len(w), 3)).astype(np.float32)
    for t in (a, b):
        t.set_touches(w, bd)
        t.set_sensors(w, bd, p=(0.0, 0.0, 0.0), d=d, dt=4.0)
    U = RC.controls(u, planted)
    _rollout(a, U, dt, iters, IMPULSE, None, names=("x",))
    _loop(b, U, dt, iters, IMPULSE, None, names=("x",))
    assert a.counter("capacity_retries") > 0

    def readers(t):
        return [t.read_touches().tobytes(), t.cast_sensors().tobytes(), t.body_contacts().tobytes()]
    ra = readers(a)
    assert ra == readers(b) and not _same(a, b)
    from mgf_amd import _capi
    assert np.frombuffer(ra[0], _capi.TOUCH_REPORT_DTYPE)["n_contacts"].sum() > 0     # the sensors have something to report
    ud = _dev(U[1])
    for t in (a, b):
        t.actuate_dev(ud, IMPULSE)
        t.step(dt, iters, 1)
    assert readers(a) == readers(b) and not _same(a, b)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_that_need_the_handle_leave_the_batch_as_it_was(ctx):
    import mgf_amd
    import torch
    from mgf_amd import _capi
    INV = _capi.ERR_INVALID
    (a, b, c), scs, rig, u, planted = _late_twins(ctx, 3, cons_per_body_of_first=None)
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    lib = mgf_amd.load_library()
    n, T, total = len(rig), 3, len(a)
    m = 5
    dev = torch.zeros(T * n + m + 13 * T * m + 64, dtype=torch.float32, device="cuda")
    _sync()
    up = dev.data_ptr()
    bp = up + 4 * T * n
    xp = bp + 4 * m
    qp, vp, op = xp + 12 * T * m, xp + 28 * T * m, xp + 40 * T * m
    stats = (_capi.StepStats * (T * a.n_worlds))()
    U = np.zeros((T, n), np.float32)
    body = np.zeros(m, np.int32)
    x = np.zeros((T, m, 3), np.float32)

    def err():
        return lib.mgf_last_error().decode()

    def dev_call(n_ticks=T, u=up, n_act=n, mode=IMPULSE, body=bp, m=m, x=xp, q=qp, v=vp, om=op):
        return lib.mgf_batch_rollout_dev(a._h, dt, iters, n_ticks, u, n_act, mode, body, m, x, q, v, om, stats)

    def host_call(n_ticks=T, u=U.ctypes.data, n_act=n, mode=IMPULSE, body=body.ctypes.data, m=m):
        return lib.mgf_batch_rollout(a._h, dt, iters, n_ticks, u, n_act, mode, body, m, x.ctypes.data, None, None, None, stats)
    for call in (dev_call, host_call):
        for wrong in (n - 1, n + 1, 0):
            assert call(n_act=wrong) == INV and "actuator_count" in err(), wrong
        assert call(u=None) == INV and "NULL" in err()
        assert call(body=None, m=total + 1) == INV and "number of bodies" in err()
        assert call(mode=2) == INV and "mode" in err()
        assert call(n_ticks=(1 << 20) + 1) == INV and "2^20" in err()
    # the device form's own: outputs that overlap each other or an input (all of it device memory: nothing here hands the call a
    # host pointer)
    assert dev_call(n_ticks=T + 1) == INV and "overlaps" in err()               # every array T + 1 rows long: they run into each other
    assert dev_call(q=xp + 12 * T * m - 4) == INV and "overlaps" in err()
    assert dev_call(v=qp) == INV and "overlaps" in err()
    assert dev_call(x=up + 4 * T * n - 4) == INV and "overlaps" in err()          # x over the end of u
    assert dev_call(om=bp) == INV and "overlaps" in err()                       # omega over body
    _sync()
    assert not dev.any().item() and not x.any()                                  # nothing was written
    assert not _same(a, c) and not _same(b, c)
    # and the batch is as it was: the next rollout is the twin's loop
    U = RC.controls(u, planted)
    got, got_stats = _rollout(a, U, dt, iters, IMPULSE, None)
    want, want_stats = _loop(b, U, dt, iters, IMPULSE, None)
    assert got == want and got_stats == want_stats and not _same(a, b)
