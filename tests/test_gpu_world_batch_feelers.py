"""The body-mounted feelers of a batch (mgf_batch_set_feelers / _cast_feelers / _cast_feelers_dev; WorldBatch.set_feelers /
.cast_feelers / .cast_feelers_dev) against their definition on the SAME batch at the same moment: the casts equal the numpy
restatement over state() and colliders() byte for byte (tests/batch_feeler_cases.py, held to the oracle by
tests/test_world_batch_feelers_host.py), and the hits equal WorldBatch.sweep of those casts byte for byte - sweep is itself held to the
lone world and the oracle by the tests of the queries - on bodies that have turned, under every mask, through the host form and the
device form; a feeler follows write_state at once and its own shape at the next tick; the rig stays on the bodies it named when bodies
are added; the launch counts are the header's; what needs the handle is refused with the rig as it was; nothing else changes."""
import numpy as np
import pytest

from tests import batch_feeler_cases as FC
from tests import batch_sensor_cases as SC

pytestmark = pytest.mark.gpu
BODIES, TERRAIN, OBSTACLES, ALL = 1, 2, 4, 7
MASKS = (BODIES, TERRAIN, OBSTACLES, ALL)


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


def _make(ctx, scs):
    import mgf_amd
    return mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)


def _step(b, scs, n=1):
    b.step(float(scs[0]["dt"]), scs[0]["iters"], n)


def _spin(b, seed):
    """angular velocities for every body (the linear ones kept): q leaves the identity within a tick"""
    lens = _lengths(b)
    w = np.concatenate([np.full(n, k, np.int32) for k, n in enumerate(lens)])
    bd = np.concatenate([np.arange(n, dtype=np.int32) for n in lens])
    om = np.random.default_rng(seed).uniform(-9.0, 9.0, (len(w), 3)).astype(np.float32)
    b.set_velocities(w, bd, b.get(w, bd)["linear"], om)


def _assert_turned(b):
    q = b.state()["q"]
    away = np.sum(q != np.float32([1, 0, 0, 0]), axis=1) >= 2
    assert 2 * int(np.sum(away)) >= len(q), (int(np.sum(away)), len(q))      # a rig on unrotated bodies tests nothing of rotate


def _turned(ctx, seed=5):
    scs = FC.feeler_scenes()
    b = _make(ctx, scs)
    _spin(b, seed)
    _step(b, scs, FC.TICKS)
    _assert_turned(b)
    return b, scs


def _reference(b, rig, kinds):
    """(hits, casts) by the definition: the restatement's casts from state() and colliders(), through sweep"""
    c = FC.casts(rig, b.state(), b.colliders(), _lengths(b))
    return b.sweep(rig["world"], c, None, ignore=FC.ignore_of(rig), kinds=kinds), c


def _cast_dev(b, kinds, casts=True):
    """cast_feelers_dev between two waits for the whole device; `out` and `casts` start as 0x5A bytes: a record the call does not
    write shows"""
    import torch
    from mgf_amd._capi import MOVING_DTYPE, SWEEP_HIT_DTYPE
    n = b.feeler_count()
    out = torch.full((n, 13), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    cs = torch.full((n, 11), 0x5A5A5A5A, dtype=torch.int32, device="cuda").view(torch.float32) if casts else None
    _sync()
    b.cast_feelers_dev(out, kinds=kinds, casts=cs)
    _sync()
    return out.cpu().numpy().view(SWEEP_HIT_DTYPE).reshape(n), (cs.cpu().numpy().view(MOVING_DTYPE).reshape(n) if casts else None)


def _where(got, want):
    """the first records that differ"""
    return [i for i in range(len(got)) if got[i].tobytes() != want[i].tobytes()][:8]


def _assert_casts(b, kinds, want, want_casts, note):
    got, cs = b.cast_feelers(kinds, casts=True)
    assert cs.tobytes() == want_casts.tobytes(), (note, kinds, "casts, host form", _where(cs, want_casts))
    assert got.tobytes() == want.tobytes(), (note, kinds, "host form", _where(got, want))
    assert b.cast_feelers(kinds).tobytes() == want.tobytes(), (note, kinds, "host form without casts")
    got, cs = _cast_dev(b, kinds)
    assert cs.tobytes() == want_casts.tobytes(), (note, kinds, "casts, device form", _where(cs, want_casts))
    assert got.tobytes() == want.tobytes(), (note, kinds, "device form", _where(got, want))
    got, _ = _cast_dev(b, kinds, casts=False)
    assert got.tobytes() == want.tobytes(), (note, kinds, "device form without casts", _where(got, want))


def _assert_parity(b, rig, note, masks=MASKS):
    ref = {}
    for m in masks:
        ref[m] = _reference(b, rig, m)
        _assert_casts(b, m, ref[m][0], ref[m][1], note)
    return ref


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_hits_and_casts_equal_the_definition_byte_for_byte(ctx):
    b, scs = _turned(ctx)
    lay = FC.main_layout(scs)
    rig = FC.aimed_rig(lay, scs, b.state(), _lengths(b))
    assert b.feeler_count() == 0
    b.set_feelers(rig)
    assert b.feeler_count() == len(rig) and 900 <= len(rig) <= 1100
    ref = _assert_parity(b, rig, "main")
    want, want_casts = ref[ALL]
    # the conditions of the test, from the REFERENCE's answers alone
    kinds = want["kind"]
    counts = {k: int(np.sum(kinds == k)) for k in (-1, 0, 1, 2)}
    print("reference kinds under QUERY_ALL:", counts)
    assert set(kinds.tolist()) == {-1, 0, 1, 2} and min(counts.values()) >= 20, counts
    hit = kinds >= 0
    assert set(rig["flags"][hit].tolist()) == set(FC.ALLOWED_FLAGS), sorted(set(rig["flags"][hit].tolist()))
    assert np.any(hit & (want["t"] == 0.0)) and np.any(hit & (want["t"] > 0.0) & (want["t"] < 1.0))
    assert set(rig["tag"][hit & ((rig["flags"] & FC.OWN_SHAPE) == 0)].tolist()) == {0, 1}
    assert np.any(hit & np.all(rig["delta"] == 0, axis=1))                                            # a zero delta that meets something
    one = (rig["world"] == FC.ONE_BODY_WORLD) & ((rig["flags"] & FC.IGNORE_SELF) != 0)
    assert np.any(one) and not np.any(kinds[one] == 0)                                                # alone in its world, itself ignored
    assert set(ref[BODIES][0]["kind"].tolist()) == {-1, 0} and set(ref[TERRAIN][0]["kind"].tolist()) == {-1, 1} and set(ref[OBSTACLES][0]["kind"].tolist()) == {-1, 2}
    # an OWN_SHAPE feeler casts colliders(world)[body] as it stands
    own = np.flatnonzero(rig["flags"] & FC.OWN_SHAPE)
    off = SC.offsets(_lengths(b))
    col = b.colliders()[off[rig["world"][own]] + rig["body"][own]]
    for k in ("tag", "p", "d", "r"):
        assert want_casts[k][own].tobytes() == col[k].tobytes(), k
    assert len(own) >= 100 and np.sum(kinds[own] >= 0) >= 20
    # the rig given in reversed order: the same answers, feeler by feeler; and through the arrays of set_feelers
    b.set_feelers(rig[::-1].copy())
    _assert_casts(b, ALL, want[::-1].copy(), want_casts[::-1].copy(), "reversed")
    f = rig["flags"]
    b.set_feelers(rig["world"], rig["body"], rig["tag"], rig["p"], rig["d"], rig["r"], rig["delta"], (f & 1) != 0, (f & 2) != 0, (f & 4) != 0)
    _assert_casts(b, ALL, want, want_casts, "by arrays")


def test_own_shapes_under_a_mask_without_bodies_against_the_lone_worlds(ctx):
    """Two worlds of three bodies, one of them a capsule; every body carries a feeler of its own shape and an ordinary one.  The casts
    and the hits under a mask of terrain only - nothing of the bodies is staged then, and an own shape is still the body's collider
    row - and under bodies and terrain equal mgf_world_sweep_many of the lone worlds byte for byte, at tick 0, when the lone worlds'
    state is the batch's by construction."""
    import mgf_amd
    from mgf_amd import scenes
    f32 = np.float32
    scs = [FC._capsuled(scenes.sphere_pile(3, 1, 1, seed=311 + k), k) for k in range(2)]
    b = _make(ctx, scs)
    lone = [mgf_amd.World.from_scene(ctx, sc) for sc in scs]
    assert _lengths(b) == [3, 3] and [len(w) for w in lone] == [3, 3]
    assert [int(np.sum(b.colliders(k)["tag"] == 1)) for k in range(2)] == [1, 1]
    n = 12
    world, body = np.repeat(np.int32([0, 1]), 6), np.tile(np.repeat(np.int32([0, 1, 2]), 2), 2)
    own = np.arange(n) % 2 == 0                                          # feeler 2j: body j's own shape; 2j + 1: a thin sphere from above it
    p = np.tile(f32([0.0, 0.9, 0.0]), (n, 1))
    delta = np.where(own[:, None], f32([0.8, 0.4, 0.0]), f32([0.0, -3.0, 0.0])).astype(f32)
    b.set_feelers(world, body, np.zeros(n, np.int32), p, np.zeros((n, 3), f32), np.full(n, 0.1, f32), delta, ignore_self=own, world_delta=True, own_shape=own)
    ign = np.where(own, body, -1).astype(np.int32)
    seen = {}
    for kinds in (TERRAIN, BODIES | TERRAIN):
        hits, casts = b.cast_feelers(kinds, casts=True)
        for k in range(2):
            sel = world == k
            want = lone[k].sweep(casts[sel], ignore=ign[sel], kinds=kinds)
            assert hits[sel].tobytes() == want.tobytes(), (kinds, k, _where(hits[sel], want))
        got, cs = _cast_dev(b, kinds)
        assert got.tobytes() == hits.tobytes() and cs.tobytes() == casts.tobytes(), kinds
        seen[kinds] = (hits, casts)
    assert seen[TERRAIN][1].tobytes() == seen[BODIES | TERRAIN][1].tobytes()       # the casts do not depend on the mask
    casts = seen[TERRAIN][1]
    col = b.colliders()[3 * world + body]
    for key in ("tag", "p", "d", "r"):                                   # an own shape: the collider row as it stands, capsule and spheres
        assert casts[key][own].tobytes() == col[key][own].tobytes(), key
    assert sorted(casts["tag"][own].tolist()) == [0, 0, 0, 0, 1, 1] and np.all(casts["r"][own] >= f32(0.4))
    # the conditions of the case, from the lone worlds' answers: the thin spheres above the sphere bodies (whose q is the identity)
    # meet the floor, or - where bodies are asked for - a body
    thin = ~own & (col["tag"] == 0)
    assert int(np.sum(thin)) == 4 and set(seen[TERRAIN][0]["kind"].tolist()) <= {-1, 1} and np.all(seen[TERRAIN][0]["kind"][thin] == 1)
    assert np.all(seen[BODIES | TERRAIN][0]["kind"][thin] == 0)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_items_of_one_of_256_of_257_and_of_600_feelers(ctx):
    """one feeler on 256 lanes (the reduction across waves), a full item, an item of one behind a full one, three items"""
    b, scs = _turned(ctx, seed=6)
    lay = FC.plan_layout(scs)
    assert np.bincount(lay["world"], minlength=5).tolist() == list(SC.PLAN_COUNTS)
    rig = FC.aimed_rig(lay, scs, b.state(), _lengths(b), seed=98)
    b.set_feelers(rig)
    ref = _assert_parity(b, rig, "plan", masks=(ALL, BODIES))
    kinds = ref[ALL][0]["kind"]
    for w, c in enumerate(SC.PLAN_COUNTS):
        if c >= 256:
            assert np.any(kinds[rig["world"] == w] >= 0), w            # the worlds of more than one wave a feeler meet something
    assert int(np.sum(rig["world"] == 1)) == 1                         # the one feeler that has all 256 lanes


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_pose_moves_a_feeler_at_once_and_its_own_shape_at_the_next_tick(ctx):
    b, scs = _turned(ctx, seed=7)
    lay = FC.main_layout(scs)
    rig = FC.aimed_rig(lay, scs, b.state(), _lengths(b))
    b.set_feelers(rig)
    k = FC.PILE_WORLD
    st, col_before = b.state(k), b.colliders()
    before, casts_before = b.cast_feelers(ALL, casts=True)
    rng = np.random.default_rng(8)
    q = rng.normal(0, 1, st["q"].shape)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    x = (st["x"] + rng.uniform(-0.2, 0.2, st["x"].shape)).astype(np.float32)
    b.write_state(k, x=x, q=q)
    assert np.array_equal(b.state(k)["q"], q) and b.colliders().tobytes() == col_before.tobytes()     # the colliders have not moved
    want, want_casts = _reference(b, rig, ALL)
    here = rig["world"] == k
    own = here & ((rig["flags"] & FC.OWN_SHAPE) != 0)
    plain = here & ~own
    assert np.all(np.any(want_casts["p"][plain] != casts_before["p"][plain], axis=1))                  # the NEW pose, at once
    for f in ("tag", "p", "d", "r"):                                                                  # the OLD collider ...
        assert want_casts[f][own].tobytes() == casts_before[f][own].tobytes(), f
    turned = own & ((rig["flags"] & FC.WORLD_DELTA) == 0)
    assert np.all(np.any(want_casts["delta"][turned] != casts_before["delta"][turned], axis=1))       # ... along a delta turned by the NEW q
    assert want_casts[~here].tobytes() == casts_before[~here].tobytes() and want.tobytes() != before.tobytes()
    _assert_casts(b, ALL, want, want_casts, "behind write_state")
    _step(b, scs)                                                                                     # the next tick moves the colliders
    assert b.colliders().tobytes() != col_before.tobytes()
    want, want_casts = _reference(b, rig, ALL)
    assert np.any(want_casts["p"][own] != casts_before["p"][own])
    _assert_casts(b, ALL, want, want_casts, "a tick behind write_state")


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_bodies_added_to_a_middle_world_leave_every_feeler_on_its_body_and_an_empty_rig_casts_nothing(ctx):
    import torch
    from mgf_amd import _capi
    b, scs = _turned(ctx, seed=9)
    lay = FC.main_layout(scs)
    rig = FC.aimed_rig(lay, scs, b.state(), _lengths(b))
    b.set_feelers(rig)
    _assert_parity(b, rig, "before add_bodies", masks=(ALL,))
    old = SC.offsets(_lengths(b))
    mid = scs[FC.ONE_BODY_WORLD]
    comps = mid["comps"][:1].repeat(2)
    comps["p"] += np.float32([[0.0, 1.5, 0.0], [0.0, 3.0, 0.0]])
    b.add_bodies(FC.ONE_BODY_WORLD, comps, 1.0, float(mid["restitution"][0]), float(mid["friction"][0]), mid["force"][:1].repeat(2, axis=0))
    assert _lengths(b) == [5, 3, 300, 48, 18] and b.feeler_count() == len(rig)
    assert np.any(SC.offsets(_lengths(b))[rig["world"]] != old[rig["world"]])          # flat indices have moved under the rig
    _assert_parity(b, rig, "behind add_bodies", masks=(ALL,))                          # the reference names the same (world, body)
    _step(b, scs)
    ref = _assert_parity(b, rig, "a tick behind add_bodies", masks=(ALL,))
    assert np.any(ref[ALL][0]["kind"] >= 0)
    # n = 0 empties the rig; a cast then enqueues nothing
    b.set_feelers(np.zeros(0, _capi.FEELER_DTYPE))
    assert b.feeler_count() == 0
    assert len(b.cast_feelers(ALL)) == 0 and b.counter("query_launches") == 0
    hits, casts = b.cast_feelers(ALL, casts=True)
    assert len(hits) == 0 and len(casts) == 0
    b.cast_feelers_dev(torch.zeros((0, 13), dtype=torch.int32, device="cuda"))
    assert b.counter("query_launches") == 0


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_launch_counts(ctx):
    from mgf_amd import _capi
    L = _capi.BATCH_FEELER_LAUNCHES
    all_scs = FC.feeler_scenes()
    for worlds in ((FC.PILE_WORLD, FC.TERRAIN_WORLD), tuple(range(len(all_scs)))):     # the pile has a mesh and a ring
        scs = [all_scs[k] for k in worlds]
        b = _make(ctx, scs)
        lens = _lengths(b)
        world = np.int32([k % len(scs) for k in range(700)])
        body = np.int32([k % lens[w] for k, w in enumerate(world)])
        for n in (1, 700):
            b.set_feelers(world[:n], body[:n], tag=0, r=0.1, delta=(0.0, -1.0, 0.0))
            got = []
            for m in (BODIES, BODIES | TERRAIN, BODIES | OBSTACLES, ALL, TERRAIN, OBSTACLES):
                b.cast_feelers(m)
                got.append(b.counter("query_launches"))
                _cast_dev(b, m)
                got.append(b.counter("query_launches"))
            assert got == [L, L, L + 1, L + 1, L + 1, L + 1, L + 2, L + 2, L + 1, L + 1, L + 1, L + 1], (worlds, n, got)
        _step(b, scs)
        _cast_dev(b, ALL)
        assert b.counter("query_launches") == L + 2 + 1                                # the collider gather behind a step, once
        _cast_dev(b, ALL)
        assert b.counter("query_launches") == L + 2
        _step(b, scs)
        b.cast_feelers(BODIES)
        assert b.counter("query_launches") == L + 1
        b.cast_feelers(BODIES)
        assert b.counter("query_launches") == L
        assert b.counter("device_skipped") == 0


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_that_need_the_handle_leave_the_rig_as_it_was(ctx):
    import mgf_amd
    import torch
    from mgf_amd import _capi
    from tests import batch_parts_cases as PC
    INV = _capi.ERR_INVALID
    b, scs = _turned(ctx, seed=10)
    lay = FC.main_layout(scs)
    rig = FC.aimed_rig(lay, scs, b.state(), _lengths(b))
    b.set_feelers(rig)
    n, K, lens = len(rig), b.n_worlds, _lengths(b)
    kept = b.cast_feelers(ALL)
    lib = mgf_amd.load_library()
    plain = int(np.flatnonzero(rig["flags"] == FC.IGNORE_SELF)[0])
    own = int(np.flatnonzero(rig["flags"] & FC.OWN_SHAPE)[0])
    cases = [(plain, "world", -1), (plain, "world", K), (plain, "body", -1), (plain, "body", lens[int(rig["world"][plain])]), (plain, "flags", 8), (plain, "flags", 9),
             (plain, "flags", -1), (plain, "tag", 2), (plain, "tag", -1), (own, "flags", FC.OWN_SHAPE), (own, "flags", FC.OWN_SHAPE | FC.WORLD_DELTA),
             (plain, "reserved", (1, 0)), (own, "reserved", (0, -1))]
    for at, field, value in cases:
        bad = rig.copy()
        bad[field][at] = value
        with pytest.raises(mgf_amd.MgfError) as e:
            b.set_feelers(bad)
        assert e.value.status == INV and "the rig was not changed" in str(e.value) and b.feeler_count() == n, (field, value, str(e.value))
    ok = rig.copy()
    ok["tag"][own] = 2                                                                 # with OWN_SHAPE the tag is not read
    b.set_feelers(ok)
    b.set_feelers(rig)
    out = np.zeros(n, _capi.SWEEP_HIT_DTYPE)
    assert lib.mgf_batch_cast_feelers(b._h, ALL, out.ctypes.data, None, n - 1) == _capi.ERR_CAPACITY
    assert lib.mgf_batch_cast_feelers(b._h, ALL, None, None, n) == INV                 # (a rig that is not empty needs somewhere to go)
    assert lib.mgf_batch_cast_feelers_dev(b._h, ALL, None, None, n) == INV
    dev = torch.zeros((n, 13 + 11), dtype=torch.int32, device="cuda")
    _sync()
    assert lib.mgf_batch_cast_feelers_dev(b._h, ALL, dev.data_ptr(), None, n - 1) == _capi.ERR_CAPACITY
    host_casts = np.zeros(n, _capi.MOVING_DTYPE)
    assert lib.mgf_batch_cast_feelers_dev(b._h, ALL, out.ctypes.data, None, n) == INV and "out_dev" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_cast_feelers_dev(b._h, ALL, dev.data_ptr(), host_casts.ctypes.data, n) == INV and "casts_out_dev" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_cast_feelers_dev(b._h, ALL, dev.data_ptr(), dev.data_ptr() + 52 * n - 4, n) == INV and "overlaps" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_cast_feelers_dev(b._h, ALL, dev.data_ptr() + 44 * n - 4, dev.data_ptr(), n) == INV and "overlaps" in lib.mgf_last_error().decode()
    _sync()
    assert not dev.any().item()                                                        # nothing was written
    assert b.feeler_count() == n and b.cast_feelers(ALL).tobytes() == kept.tobytes()
    # a batch that holds a dumbbell: set_feelers stays as it is, both casts are refused, and the next step still matches the twin's
    dsc = [PC.six_scenes()[PC.DUMBBELLS]]
    a, d = _make(ctx, dsc), _make(ctx, dsc)
    d.set_feelers(0, [0, 1], tag=0, r=0.1, delta=(0.0, -1.0, 0.0))
    assert d.feeler_count() == 2
    two = np.zeros(2, _capi.SWEEP_HIT_DTYPE)
    dev2 = torch.zeros((2, 13), dtype=torch.int32, device="cuda")
    _sync()
    assert lib.mgf_batch_cast_feelers(d._h, ALL, two.ctypes.data, None, 2) == INV and "several components" in lib.mgf_last_error().decode()
    assert lib.mgf_batch_cast_feelers_dev(d._h, ALL, dev2.data_ptr(), None, 2) == INV and "several components" in lib.mgf_last_error().decode()
    _step(a, dsc)
    _step(d, dsc)
    sa, sd = a.state(), d.state()
    assert all(sa[f].tobytes() == sd[f].tobytes() for f in ("x", "q", "v", "omega", "delta")) and a.constraints(0).tobytes() == d.constraints(0).tobytes()


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def _everything(b):
    st = b.state()
    return [st[k].tobytes() for k in ("x", "q", "v", "omega", "delta")] + [b.constraints(k).tobytes() for k in range(b.n_worlds)]


def test_nothing_else_changes(ctx):
    """the other rigs of the same batch answer the same bytes before and after feeler casts; state and constraint lists are untouched,
    and the next step is the twin's"""
    from mgf_amd import _capi
    scs = FC.feeler_scenes()
    a, b = _make(ctx, scs), _make(ctx, scs)
    for t in (a, b):
        _spin(t, 11)
        _step(t, scs, FC.TICKS)
    assert _everything(a) == _everything(b)
    lay = FC.main_layout(scs)
    lens = _lengths(b)
    b.set_sensors(SC.aimed_rig(dict(lay, role=np.where(lay["role"] == FC.DOWN, SC.DOWN, SC.RANDOM)), scs, b.state(), lens))
    b.set_zones(lay["world"][:200], lay["body"][:200], (0.0, 0.0, 0.0), (0.8, 0.8, 0.8), True)
    b.set_touches(lay["world"][:200], lay["body"][:200], _capi.TOUCH_ANY)

    def others():
        s, pt = b.cast_sensors(ALL, parts=True)
        cnt, bodies = b.read_zones(4)
        return [s.tobytes(), pt.tobytes(), cnt.tobytes(), bodies.tobytes(), b.read_touches().tobytes()]
    before = others()
    b.set_feelers(FC.aimed_rig(lay, scs, b.state(), lens))
    for m in (ALL, BODIES | TERRAIN):
        b.cast_feelers(m, casts=True)
        _cast_dev(b, m)
    assert others() == before
    assert b.sensor_count() == len(lay["world"]) and b.zone_count() == 200 and b.touch_count() == 200
    assert _everything(a) == _everything(b)            # (a cast writes nothing a reader of the state sees)
    _step(a, scs)
    _step(b, scs)
    _cast_dev(b, ALL)
    assert _everything(a) == _everything(b)
