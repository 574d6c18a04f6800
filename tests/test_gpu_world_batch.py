"""Many small worlds in one batch (mgf_batch_*, DESIGN.md "many small worlds"): every world of a batch against its own oracle world
(World(ORDER_CANONICAL), the definition) and against the lone mgf_world, bit for bit - state, constraint list with impulses, the tick's
counts - wherever the world sits in the batch and whatever else the batch holds."""
import ctypes as C

import numpy as np
import pytest

from mgf_amd import scenes
from oracle import oracle as O
from tests import contact_corpus as CC
from tests.util import bits_equal, compare_constraints, oracle_world

pytestmark = pytest.mark.gpu

STATE = ("x", "q", "v", "omega", "delta")
COUNTS = ("n_constraints", "n_terrain_constraints", "n_pair_candidates", "n_refits")


@pytest.fixture(scope="module")
def ctx():
    import mgf_amd
    c = mgf_amd.Context(0)
    yield c
    c.close()


def _empty_scene(terrain):
    sc = scenes.sphere_pile(1, 1, 1)
    return dict(sc, name="empty", comps=sc["comps"][:0], mass=sc["mass"][:0], restitution=sc["restitution"][:0], friction=sc["friction"][:0],
                force=sc["force"][:0], v0=None, terrain=terrain)


def pile_scenes():
    """the heterogeneous worlds of tests 1, 4, 5, 6, 7 over one box: 512, 1000, 96, 512 (another seed), 0 and 1 bodies"""
    big = scenes.sphere_pile(10, 10, 10)
    out = [scenes.sphere_pile(8, 8, 8), big, scenes.sphere_pile(4, 6, 4, seed=5), scenes.sphere_pile(8, 8, 8, seed=77), None, scenes.sphere_pile(1, 1, 1)]
    out[4] = _empty_scene(big["terrain"])
    return [dict(sc, terrain=big["terrain"]) for sc in out]


def _same_state(got, want, what):
    for f in STATE:
        assert bits_equal(got[f], want[f]), f"{what}: {f} differs"


def _same_counts(st, ost, what):
    for f in COUNTS:
        assert getattr(st, f) == getattr(ost, f), f"{what}: {f} = {getattr(st, f)}, the oracle has {getattr(ost, f)}"


def _run_against_oracle(ctx, scs, ticks, list_ticks, terrain_scene=None):
    """the batch of `scs` free running beside one oracle world per scene; returns the most constraints each world saw and the last stats"""
    import mgf_amd
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs)
    ows = [oracle_world(sc) for sc in scs]
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    seen = [0] * len(scs)
    seen_t = [0] * len(scs)
    seen_p = [0] * len(scs)
    for tick in range(1, ticks + 1):
        st = b.step(dt, iters)
        for k, ow in enumerate(ows):
            ost = ow.step(dt, iters)
            what = f"world {k} tick {tick}"
            assert st[k].n_bodies == len(scs[k]["comps"]) and st[k].iters == iters
            _same_counts(st[k], ost, what)
            _same_state(b.state(k), ow.state(), what)
            if tick in list_ticks:
                compare_constraints(b.constraints(k), ow.constraints(), check_impulse=True)
            seen[k] = max(seen[k], int(ost.n_constraints))
            seen_t[k] = max(seen_t[k], int(ost.n_terrain_constraints))
            seen_p[k] = max(seen_p[k], int(ost.n_constraints - ost.n_terrain_constraints))
    return b, seen, seen_t, seen_p


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_heterogeneous_piles_against_the_oracle_free_running(ctx):
    scs = pile_scenes()
    b, seen, _, _ = _run_against_oracle(ctx, scs, 120, (1, 2, 10, 60, 120))
    print("most constraints per world:", seen, "capacity_retries:", b.counter("capacity_retries"))
    assert all(seen[k] > 100 for k in (0, 1, 2, 3)), seen
    whole = b.state()
    assert len(whole["x"]) == len(b) == sum(len(sc["comps"]) for sc in scs)
    at = 0
    for k, sc in enumerate(scs):
        assert b.world_len(k) == len(sc["comps"])
        _same_state({f: whole[f][at:at + len(sc["comps"])] for f in STATE}, b.state(k), f"world {k} of the whole-batch read")
        at += len(sc["comps"])


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_capsules_and_a_heightfield(ctx):
    a, c = scenes.capsule_field(4, 3, 4), scenes.capsule_field(8, 4, 8, sphere_fraction=0.5)
    assert (len(a["comps"]), len(c["comps"])) == (48, 256)
    scs = [a, dict(c, terrain=a["terrain"])]
    b, seen, seen_t, seen_p = _run_against_oracle(ctx, scs, 200, (1, 20, 60, 200))
    print("most constraints per world:", seen, "terrain:", seen_t, "pairs:", seen_p)
    assert all(t > 0 for t in seen_t) and all(p > 0 for p in seen_p), (seen_t, seen_p)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rung", CC.WORLD_RUNGS, ids=[f"rung{r}" for r in CC.WORLD_RUNGS])
def test_the_contact_corpus_through_the_batch(ctx, rung):
    import mgf_amd
    K = 16
    allp = CC.plant(CC.base_cases(CC.PAIR_TYPES), rung)
    tris = CC.plant(CC.base_cases(CC.TRI_TYPES, per_family=8), rung)
    shared = CC.with_mesh(CC.pair_world(allp[:0]), tris)["mesh"]
    worlds = [dict(CC.with_mesh(CC.pair_world(allp[k::K]), tris[k::K]), mesh=shared) for k in range(K)]
    b = mgf_amd.WorldBatch(ctx, K)
    m = mgf_amd.Mesh(ctx)
    m.build(shared["verts"], shared["faces"])
    m.set_pos(shared["pos"])
    b.set_terrain(m)
    total = 0
    for k, sc in enumerate(worlds):
        assert len(sc["comps"]) <= mgf_amd.BATCH_MAX_BODIES
        b.add_bodies(k, sc["comps"], 1.0, 0.3, 0.6, (0.0, 0.0, 0.0))
        b.write_state(k, v=sc["delta"])
    st = b.step(1.0, CC.ITERS)
    for k, sc in enumerate(worlds):
        what = f"rung {rung} world {k}"
        ow = CC.oracle_world(sc)
        recount = CC.LeafRecount(ow)
        ow.set_state(v=sc["delta"])
        ost = ow.step(1.0, CC.ITERS)
        got, want = b.constraints(k), ow.constraints()
        assert len(got) == len(want), what
        assert np.array_equal(got["a"], want["a"]) and np.array_equal(got["b"], want["b"]), what
        for f in ["normal", "t0", "t1", "ra", "rb", "bias", "normal_mass", "tangent_mass0", "tangent_mass1", "friction", "normal_impulse"]:
            assert CC.same_f32(got[f], want[f]), f"{what}: constraint field {f} differs"
        g, o = b.state(k), ow.state()
        for f in STATE:
            assert CC.same_f32(g[f], o[f]), f"{what}: {f} differs"
        assert (st[k].n_constraints, st[k].n_terrain_constraints) == (ost.n_constraints, ost.n_terrain_constraints), what
        leaves = recount.count(ow)
        if st[k].n_pair_candidates != ost.n_pair_candidates:  # the one stated limit (include/mgf_hip.h at mgf_step_stats): by the leaf boxes, 1e5 from the origin
            assert CC.LADDER[rung][0] >= 1e5 and st[k].n_pair_candidates == leaves > ost.n_pair_candidates, what
        else:
            assert leaves == st[k].n_pair_candidates, what
        assert ost.n_constraints > 100, (what, ost.n_constraints)
        total += int(ost.n_constraints)
    print(f"rung {rung}: {total} constraints in {K} worlds, capacity_retries {b.counter('capacity_retries')}")


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_against_the_lone_world(ctx):
    import mgf_amd
    scs = pile_scenes()
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs)
    lone = [mgf_amd.World.from_scene(ctx, sc) for sc in scs]
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    for tick in range(1, 61):
        b.step(dt, iters)
        for w in lone:
            if len(w):
                w.step(dt, iters)
        if tick in (1, 10, 60):
            for k, w in enumerate(lone):
                _same_state(b.state(k), w.state(), f"world {k} tick {tick}")
                if len(w):
                    compare_constraints(b.constraints(k), w.constraints(), check_impulse=True)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_a_world_does_not_depend_on_its_batch(ctx):
    import mgf_amd
    scs = pile_scenes()
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]

    def run(sub):
        b = mgf_amd.WorldBatch.from_scenes(ctx, sub)
        b.step(dt, iters, 60)
        return [(b.state(k), b.constraints(k)) for k in range(len(sub))]
    base = run(scs)
    rev = run(scs[::-1])[::-1]
    for k, sc in enumerate(scs):
        alone = run([sc])[0]
        for other, name in ((rev[k], "reversed"), (alone, "alone")):
            _same_state(other[0], base[k][0], f"world {k} {name}")
            compare_constraints(other[1], base[k][1], check_impulse=True)


def test_more_worlds_than_compute_units(ctx):
    import mgf_amd
    K = 300
    sc = scenes.sphere_pile(4, 6, 4)
    b = mgf_amd.WorldBatch.from_scenes(ctx, [sc] * K)
    assert b.counter("launches_per_tick") == mgf_amd.WorldBatch.from_scenes(ctx, [sc]).counter("launches_per_tick")   # (test 9: the launch cost)
    n = len(sc["comps"])
    rng = np.random.default_rng(3)
    v0 = rng.uniform(-1.0, 1.0, (K, n, 3)).astype(np.float32)
    for k in range(K):
        b.write_state(k, v=v0[k])
    dt, iters = float(sc["dt"]), sc["iters"]
    b.step(dt, iters, 30)
    whole = b.state()
    for k in range(K):
        ow = oracle_world(dict(sc, v0=v0[k]))
        for _ in range(30):
            ow.step(dt, iters)
        _same_state({f: whole[f][k * n:(k + 1) * n] for f in STATE}, ow.state(), f"copy {k}")
        if k % 50 == 0:
            compare_constraints(b.constraints(k), ow.constraints(), check_impulse=True)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_reset_of_one_world(ctx):
    import mgf_amd
    scs = pile_scenes()
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    b, ref = mgf_amd.WorldBatch.from_scenes(ctx, scs), mgf_amd.WorldBatch.from_scenes(ctx, scs)
    ow = oracle_world(scs[1])
    start = b.state(1)
    zero = np.zeros_like(start["delta"])
    b.step(dt, iters, 40)
    ref.step(dt, iters, 40)
    for _ in range(40):
        ow.step(dt, iters)
    b.write_state(1, x=start["x"], q=start["q"], v=start["v"], omega=start["omega"], delta=zero)
    ow.set_state(x=start["x"], q=start["q"], v=start["v"], omega=start["omega"], delta=zero)
    b.step(dt, iters, 40)
    ref.step(dt, iters, 40)
    for _ in range(40):
        ow.step(dt, iters)
    _same_state(b.state(1), ow.state(), "the reset world")
    compare_constraints(b.constraints(1), ow.constraints(), check_impulse=True)
    for k in (0, 2, 3, 4, 5):
        _same_state(b.state(k), ref.state(k), f"world {k} beside the reset one")
        compare_constraints(b.constraints(k), ref.constraints(k), check_impulse=True)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_step_n_is_n_steps(ctx):
    import mgf_amd
    scs = pile_scenes()
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    a, b = mgf_amd.WorldBatch.from_scenes(ctx, scs), mgf_amd.WorldBatch.from_scenes(ctx, scs)
    sa = a.step(dt, iters, 20)
    sb = [b.step(dt, iters) for _ in range(20)]
    K = len(scs)
    assert len(sa) == 20 * K
    for t in range(20):
        for k in range(K):
            assert sa[t * K + k].as_dict() == sb[t][k].as_dict(), (t, k)
    assert sa[19 * K + 1].n_constraints > 100 and sa[19 * K + 1].n_bodies == 1000 and sa[19 * K + 1].iters == iters
    for k in range(K):
        _same_state(a.state(k), b.state(k), f"world {k}")
        compare_constraints(a.constraints(k), b.constraints(k), check_impulse=True)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_body_cap(ctx):
    import mgf_amd
    sc = scenes.sphere_pile(8, 16, 8)
    assert len(sc["comps"]) == mgf_amd.BATCH_MAX_BODIES == 1024
    b = mgf_amd.WorldBatch.from_scenes(ctx, [sc])
    with pytest.raises(mgf_amd.MgfError) as e:
        b.add_bodies(0, sc["comps"][:1], 1.0, 0.3, 0.6, (0.0, -9.8, 0.0))
    assert e.value.status == mgf_amd._capi.ERR_INVALID and "1024" in str(e.value)
    assert b.world_len(0) == 1024 and len(b) == 1024
    ow = oracle_world(sc)
    dt, iters = float(sc["dt"]), sc["iters"]
    for tick in range(10):
        st, ost = b.step(dt, iters), ow.step(dt, iters)
        _same_counts(st[0], ost, f"tick {tick}")
        _same_state(b.state(0), ow.state(), f"tick {tick}")
    compare_constraints(b.constraints(0), ow.constraints(), check_impulse=True)
    assert ost.n_constraints > 1000


def test_a_tick_that_outgrows_its_storage_is_run_again(ctx):
    """Solver::solve and World::step have no capacity failure (solver.rs:72-78): with one constraint record (and four candidates) a body
    allotted, the piles' ticks do not fit; they complete all the same, with the oracle's answer, and the re-runs are counted"""
    import mgf_amd
    scs = pile_scenes()
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs)
    b.set_option("cons_per_body", 1)
    ows = [oracle_world(sc) for sc in scs]
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    st = b.step(dt, iters, 12)
    assert b.counter("capacity_retries") > 0
    for k, ow in enumerate(ows):
        for t in range(12):
            ost = ow.step(dt, iters)
            _same_counts(st[t * len(scs) + k], ost, f"world {k} tick {t}")
        _same_state(b.state(k), ow.state(), f"world {k}")
        compare_constraints(b.constraints(k), ow.constraints(), check_impulse=True)
    assert st[11 * len(scs)].n_constraints > 512   # more than the one record a body the world started with


def test_a_batch_outlives_its_context():
    import mgf_amd
    lib = mgf_amd.load_library()
    c = mgf_amd.Context(0)
    sc = scenes.sphere_pile(2, 2, 2)
    b = mgf_amd.WorldBatch.from_scenes(c, [sc, sc])
    b.step(float(sc["dt"]), sc["iters"])
    h, b._h = b._h, None     # (Context.close would free the batch first: keep the handle out of its reach)
    c.close()
    assert lib.mgf_batch_step(h, 1.0 / 60.0, 4, 1, None) == mgf_amd._capi.ERR_INVALID
    assert "destroyed" in lib.mgf_last_error().decode()
    x = np.zeros((8, 3), np.float32)
    assert lib.mgf_batch_read_state(h, 0, x.ctypes.data, None, None, None, None, 8) == mgf_amd._capi.ERR_INVALID
    assert lib.mgf_batch_write_state(h, 0, x.ctypes.data, None, None, None, None, 8) == mgf_amd._capi.ERR_INVALID
    assert lib.mgf_batch_read_constraints(h, 0, None, 0, C.byref(C.c_int64())) == mgf_amd._capi.ERR_INVALID
    assert lib.mgf_batch_set_terrain(h, None) == mgf_amd._capi.ERR_INVALID
    lib.mgf_batch_free(h)


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------------
def test_launches_per_tick_do_not_grow_with_the_batch(ctx):
    import mgf_amd
    sc = scenes.sphere_pile(2, 2, 2)
    one, many = mgf_amd.WorldBatch.from_scenes(ctx, [sc]), mgf_amd.WorldBatch.from_scenes(ctx, [sc] * 300)
    one.step(float(sc["dt"]), 4)
    many.step(float(sc["dt"]), 4)
    assert one.counter("launches_per_tick") == many.counter("launches_per_tick") <= 8
