"""The device-pointer calls of a batch (mgf_batch_gather_state_dev, _set_many_dev, _set_forces_dev, _apply_impulses_dev,
_read_body_contacts_dev, _copy_worlds_where, mgf_ctx_synchronize) against the host-memory calls they mirror: twin batches from the same
scenes, twin A driven through mgf_batch_get_many / _set_many / _set_forces / _apply_impulses / _read_body_contacts / _copy_worlds, twin
B through the new calls with torch CUDA tensors - and everything of the two batches equal to the bit.  No test hands a host pointer or
a short buffer to a device-pointer call: the refusals are read in host_batch_dev.inc (dev_span comes before the first enqueue)."""
import os
import re

import numpy as np
import pytest

from tests import batch_device_cases as DV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import mgf_amd
    c = mgf_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scs():
    return DV.device_scenes()


@pytest.fixture(scope="module")
def set_launches():
    """the constant the header states"""
    import mgf_amd
    m = re.search(r"#define MGF_BATCH_DEV_SET_LAUNCHES (\d+)", open(os.path.join(ROOT, "include", "mgf_hip.h")).read())
    assert m and int(m.group(1)) == mgf_amd._capi.BATCH_DEV_SET_LAUNCHES
    return int(m.group(1))


def _batch(ctx, scs, ticks=0, cons_per_body=None):
    import mgf_amd
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    if cons_per_body is not None:
        b.set_option("cons_per_body", cons_per_body)
    if ticks:
        b.step(float(scs[0]["dt"]), scs[0]["iters"], ticks)
    return b


def _step(scs, *batches, n=DV.TICKS):
    for b in batches:
        b.step(float(scs[0]["dt"]), scs[0]["iters"], n)


def _everything(b, scs):
    """all the issue's "equal" covers, as bytes: read_state(-1), get of every body (force and torque rows too), colliders, every list"""
    world, body = DV.world_body(scs, np.arange(len(b)))
    st = b.state()
    out = {f: st[f].tobytes() for f in st}
    out["get"] = b.get(world, body).tobytes()
    out["colliders"] = b.colliders().tobytes()
    for k in range(b.n_worlds):
        out[f"constraints[{k}]"] = b.constraints(k).tobytes()
    return out


def _assert_same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], f"{what}: {k} differs"


def _cuda(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _sync():
    import torch
    torch.cuda.synchronize()


def _call(fn, *a, **kw):
    """a call of twin B between two waits for the whole device (the tensors come from torch's stream, the library has its own)"""
    _sync()
    r = fn(*a, **kw)
    _sync()
    return r


# ---- gather ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ticks", [0, DV.TICKS])
def test_gather_equals_get_and_read_state(ctx, scs, ticks):
    import torch
    b = _batch(ctx, scs, ticks)
    total = len(b)
    assert total == 306
    before = _everything(b, scs)
    for flat in (None, DV.subset_with_repeats(scs)):
        idx = np.arange(total) if flat is None else flat
        n = len(idx)
        world, body = DV.world_body(scs, idx)
        want, st = b.get(world, body), b.state()
        out = {k: torch.full((n, 4 if k == "q" else 3), float("nan"), dtype=torch.float32, device="cuda") for k in ("x", "q", "v", "omega", "force", "torque")}
        _call(b.gather_state, None if flat is None else _cuda(flat), **out)
        assert b.counter("drive_launches") == 1
        got = {k: t.cpu().numpy() for k, t in out.items()}
        assert got["x"].tobytes() == want["x"].tobytes()                       # x + delta
        assert got["v"].tobytes() == want["linear"].tobytes() and got["omega"].tobytes() == want["angular"].tobytes()
        assert got["force"].tobytes() == want["force"].tobytes() and got["torque"].tobytes() == want["torque"].tobytes()
        assert got["q"].tobytes() == st["q"][idx].tobytes()
        if ticks:
            assert np.any(st["delta"] != 0) and np.any(want["linear"] != 0)
        # NULL outputs are skipped: only the two asked for are written, and they come out the same
        two = {k: torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda") for k in ("omega", "force")}
        _call(b.gather_state, None if flat is None else _cuda(flat), **two)
        assert two["omega"].cpu().numpy().tobytes() == want["angular"].tobytes() and two["force"].cpu().numpy().tobytes() == want["force"].tobytes()
    ctx.synchronize()
    assert b.counter("device_skipped") == 0
    _assert_same(_everything(b, scs), before, "a gather changes nothing")


# ---- the setters ----------------------------------------------------------------------------------------------------------------------------
def test_setters_with_repeated_bodies_equal_the_host_calls(ctx, scs, set_launches):
    a, b, u = (_batch(ctx, scs, DV.TICKS) for _ in range(3))     # u: driven by nobody
    flat = DV.records(scs)
    world, body = DV.world_body(scs, flat)
    assert DV.QUIET_WORLD not in world
    d_flat = _cuda(flat)
    lin, ang = DV.rows(DV.N_RECORDS, 51, 2.0), DV.rows(DV.N_RECORDS, 52, 3.0)
    a.set_velocities(world, body, lin, ang)
    _call(b.set_velocities_dev, d_flat, _cuda(lin), _cuda(ang))
    assert b.counter("drive_launches") == set_launches
    _assert_same(_everything(b, scs), _everything(a, scs), "set_velocities_dev")
    f, t = DV.rows(DV.N_RECORDS, 53, 9.0), DV.rows(DV.N_RECORDS, 54, 4.0)
    a.set_forces(world, body, f, t)
    _call(b.set_forces_dev, d_flat, _cuda(f), _cuda(t))
    assert b.counter("drive_launches") == set_launches
    _assert_same(_everything(b, scs), _everything(a, scs), "set_forces_dev")
    il, ia = DV.impulse_rows(scs)
    a.apply_impulses(world, body, il, ia)
    _call(b.apply_impulses_dev, d_flat, _cuda(il), _cuda(ia))
    assert b.counter("drive_launches") == set_launches
    after = _everything(b, scs)
    _assert_same(after, _everything(a, scs), "apply_impulses_dev")
    # the order mattered: the triple's linear impulses sum to 1 in record order, to 0 in another
    g3 = DV.triple_body(scs)
    w3, b3 = DV.world_body(scs, np.int32([g3]))
    got = b.get(w3, b3)
    at = DV.TRIPLE_AT[-1]   # a set keeps the last record of the triple
    want_v = ((lin[at] + il[DV.TRIPLE_AT[0]] * got["inv_mass"][0]) + il[DV.TRIPLE_AT[1]] * got["inv_mass"][0]) + il[DV.TRIPLE_AT[2]] * got["inv_mass"][0]
    assert got["linear"][0].tobytes() == want_v.astype(np.float32).tobytes()
    assert got["force"][0].tobytes() == f[at].tobytes() and got["torque"][0].tobytes() == t[at].tobytes()
    # forces and torques are consumed by the next ticks' integrate
    _step(scs, a, b, u)
    _assert_same(_everything(b, scs), _everything(a, scs), "3 ticks behind the setters")
    # the world no record names is the undriven batch's, to the bit
    k = DV.QUIET_WORLD
    wq, bq = np.full(len(scs[k]["comps"]), k, np.int32), np.arange(len(scs[k]["comps"]), dtype=np.int32)
    for f_ in ("x", "q", "v", "omega", "delta"):
        assert b.state(k)[f_].tobytes() == u.state(k)[f_].tobytes(), f_
    assert b.get(wq, bq).tobytes() == u.get(wq, bq).tobytes() and b.colliders(k).tobytes() == u.colliders(k).tobytes()
    assert b.constraints(k).tobytes() == u.constraints(k).tobytes()
    assert a.get(*DV.world_body(scs, np.int32([0]))).tobytes() != u.get(*DV.world_body(scs, np.int32([0]))).tobytes()   # (the others were driven)
    assert b.counter("device_skipped") == 0


def test_setters_without_indices_and_with_one_array(ctx, scs):
    a, b = _batch(ctx, scs, DV.TICKS), _batch(ctx, scs, DV.TICKS)
    total = len(b)
    world, body = DV.world_body(scs, np.arange(total))
    lin, ang = DV.rows(total, 61, 2.0), DV.rows(total, 62, 3.0)
    # body = None: record i is body i, one launch; n may be less than the number of bodies
    a.set_velocities(world, body, lin, ang)
    _call(b.set_velocities_dev, None, _cuda(lin), _cuda(ang))
    assert b.counter("drive_launches") == 1
    _assert_same(_everything(b, scs), _everything(a, scs), "set_velocities_dev(None)")
    a.apply_impulses(world[:290], body[:290], lin[:290], None)
    _call(b.apply_impulses_dev, None, _cuda(lin[:290]), None, n=290)
    assert b.counter("drive_launches") == 1
    _assert_same(_everything(b, scs), _everything(a, scs), "apply_impulses_dev(None, n=290, angular=None)")
    a.set_forces(world, body, None, ang)
    _call(b.set_forces_dev, None, None, _cuda(ang))
    assert b.counter("drive_launches") == 1
    _assert_same(_everything(b, scs), _everything(a, scs), "set_forces_dev(None, torque only)")
    # with indices: a NULL force with a torque, and the reverse; a NULL linear with an angular impulse
    flat = DV.records(scs, seed=71)
    w, bd = DV.world_body(scs, flat)
    d_flat = _cuda(flat)
    f, t = DV.rows(len(flat), 63, 5.0), DV.rows(len(flat), 64, 5.0)
    a.set_forces(w, bd, None, t)
    _call(b.set_forces_dev, d_flat, None, _cuda(t))
    _assert_same(_everything(b, scs), _everything(a, scs), "set_forces_dev(torque only)")
    a.set_forces(w, bd, f, None)
    _call(b.set_forces_dev, d_flat, _cuda(f), None)
    _assert_same(_everything(b, scs), _everything(a, scs), "set_forces_dev(force only)")
    a.apply_impulses(w, bd, None, t)
    _call(b.apply_impulses_dev, d_flat, None, _cuda(t))
    _assert_same(_everything(b, scs), _everything(a, scs), "apply_impulses_dev(angular only)")
    _step(scs, a, b)
    _assert_same(_everything(b, scs), _everything(a, scs), "3 ticks behind")


def test_out_of_range_indices_are_skipped_whole_and_counted(ctx, scs):
    import torch
    a, b = _batch(ctx, scs, DV.TICKS), _batch(ctx, scs, DV.TICKS)
    total = len(b)
    flat = DV.records(scs, seed=81)[:300].copy()
    good = np.ones(len(flat), bool)
    flat[7], flat[290] = -1, total          # one in each block of records
    good[[7, 290]] = False
    world, body = DV.world_body(scs, flat[good])
    d_flat = _cuda(flat)
    lin, ang = DV.rows(len(flat), 82, 2.0), DV.rows(len(flat), 83, 2.0)
    skipped = b.counter("device_skipped")
    assert skipped == 0
    a.apply_impulses(world, body, lin[good], ang[good])
    _call(b.apply_impulses_dev, d_flat, _cuda(lin), _cuda(ang))
    assert b.counter("device_skipped") == skipped + 2
    _assert_same(_everything(b, scs), _everything(a, scs), "apply_impulses_dev with indices -1 and total")
    a.set_velocities(world, body, lin[good], ang[good])
    _call(b.set_velocities_dev, d_flat, _cuda(lin), _cuda(ang))
    assert b.counter("device_skipped") == skipped + 4
    _assert_same(_everything(b, scs), _everything(a, scs), "set_velocities_dev with indices -1 and total")
    # the gather: the two rows stay as they were, the others are the bodies'
    x = torch.full((len(flat), 3), -7.0, dtype=torch.float32, device="cuda")
    _call(b.gather_state, d_flat, x=x)
    assert b.counter("device_skipped") == skipped + 6
    got = x.cpu().numpy()
    assert np.all(got[~good] == -7.0) and got[good].tobytes() == a.get(world, body)["x"].tobytes()
    _assert_same(_everything(b, scs), _everything(a, scs), "gather_state with indices -1 and total")


# ---- body contacts --------------------------------------------------------------------------------------------------------------------------
def test_body_contacts_dev_equals_body_contacts(ctx, scs):
    import torch
    b = _batch(ctx, scs, DV.TICKS)
    for world in (2, None):
        want = b.body_contacts(world)
        assert len(want) == (len(b) if world is None else 300) and np.any(want.view(np.uint32) != 0)
        out = torch.full((len(want), 6), -1, dtype=torch.int32, device="cuda")
        _call(b.body_contacts_dev, out, world)
        assert b.counter("query_launches") == 1
        assert out.cpu().numpy().tobytes() == want.tobytes()


# ---- the masked copy ------------------------------------------------------------------------------------------------------------------------
def test_copy_worlds_where_equals_copy_worlds_of_the_selected_pairs(ctx, scs):
    snap = _batch(ctx, scs, DV.TICKS)                              # the snapshot: its world of 300 holds a list longer than 300 records
    a, b = _batch(ctx, scs, 0, 1), _batch(ctx, scs, 0, 1)          # cons_per_body = 1: the share of the world of 300 is 300 records
    assert len(snap.constraints(2)) > 300
    P = DV.COPY_PAIRS
    masks = {tuple(m): _cuda(np.int32(m)) for m in DV.MASKS}
    # two pairs, none grows: worlds 0 and 1 get lists
    _call(b.copy_worlds_where, [0, 1], snap, [0, 1], _cuda(np.int32([1, 1])))
    a.copy_worlds([0, 1], snap, [0, 1])
    assert b.counter("drive_launches") == 1 and b.counter("pair_table_uploads") == 1
    assert len(b.constraints(0)) > 0
    _assert_same(_everything(b, scs), _everything(a, scs), "two pairs, all selected")
    # another pair array is honoured; all zero: the share of the world of 300 grows all the same (the host cannot know the mask), the
    # lists of worlds 0 and 1 move - and B is what it was
    before = _everything(b, scs)
    _call(b.copy_worlds_where, P, snap, P, masks[(0, 0, 0)])
    assert b.counter("drive_launches") == 2 and b.counter("pair_table_uploads") == 2      # (k_batch_move_lists + the copy)
    _assert_same(_everything(b, scs), before, "all-zero mask")
    # the twins run on for two ticks; [1, 0, 1]: worlds 0 and 1 go back to the snapshot, the world of 300 - masked out - keeps its own state
    _step(scs, a, b, n=2)
    _assert_same(_everything(b, scs), _everything(a, scs), "two ticks on")
    _call(b.copy_worlds_where, P, snap, P, masks[(1, 0, 1)])
    a.copy_worlds([0, 1], snap, [0, 1])
    assert b.counter("pair_table_uploads") == 2 and b.counter("drive_launches") == 1     # the same arrays: no upload
    _assert_same(_everything(b, scs), _everything(a, scs), "mask [1, 0, 1]")
    assert b.state(2)["x"].tobytes() != snap.state(2)["x"].tobytes()
    # all one
    _call(b.copy_worlds_where, P, snap, P, masks[(1, 1, 1)])
    a.copy_worlds(P, snap, P)
    assert b.counter("pair_table_uploads") == 2
    _assert_same(_everything(b, scs), _everything(a, scs), "all-one mask")
    assert b.constraints(2).tobytes() == snap.constraints(2).tobytes()
    # the lengths of B's lists are known to the device alone: a plain copy with B as its SOURCE into shares that must grow by them
    ta, tb = _batch(ctx, scs, 0, 1), _batch(ctx, scs, 0, 1)
    b2 = _batch(ctx, scs, 0, 1)
    _call(b2.copy_worlds_where, P, snap, P, masks[(1, 1, 1)])      # (not read back in between)
    tb.copy_worlds([0, 1, 2], b2, [0, 1, 2])
    ta.copy_worlds([0, 1, 2], a, [0, 1, 2])
    _assert_same(_everything(tb, scs), _everything(ta, scs), "a plain copy out of a masked copy's destination")
    assert tb.constraints(2).tobytes() == snap.constraints(2).tobytes()
    # and all of them step on alike
    _step(scs, a, b, ta, tb)
    _assert_same(_everything(b, scs), _everything(a, scs), "3 ticks behind the copies")
    _assert_same(_everything(tb, scs), _everything(ta, scs), "3 ticks behind the plain copy")


# ---- launches -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, DV.N_RECORDS])
def test_launch_counts_do_not_depend_on_n(ctx, scs, set_launches, n):
    import torch
    b = _batch(ctx, scs, 1)
    flat = _cuda(DV.records(scs)[:n])
    r0, r1 = _cuda(DV.rows(n, 91, 1.0)), _cuda(DV.rows(n, 92, 1.0))
    out = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    m = min(n, len(b))     # without indices a call names at most every body
    s0, s1 = r0[:m], r1[:m]
    for fn, args, want in ((b.set_velocities_dev, (flat, r0, r1), set_launches), (b.set_forces_dev, (flat, r0, r1), set_launches),
                           (b.apply_impulses_dev, (flat, r0, r1), set_launches), (b.set_velocities_dev, (None, s0, s1), 1),
                           (b.set_forces_dev, (None, s0, None), 1), (b.apply_impulses_dev, (None, None, s1), 1)):
        _call(fn, *args, **({"n": m} if args[0] is None else {}))
        assert b.counter("drive_launches") == want, (fn.__name__, args[0] is None)
    _call(b.gather_state, flat, x=out)
    assert b.counter("drive_launches") == 1
    _call(b.gather_state, None, v=out[:m], n=m)
    assert b.counter("drive_launches") == 1
    ctx.synchronize()
