"""A terrain mesh and a mesh position per world of a batch (mgf_batch_add_terrain, mgf_batch_set_world_terrain): world k of the batch
against the oracle world and the lone mgf_world that hold world k's bodies over world k's terrain at world k's position, bit for bit -
the tick's state, the constraint list with impulses, the statistics, rays, sweeps, contact summaries and box overlaps - wherever the
world sits, in whatever order the table was built and whichever worlds share a mesh.  The conditions on these inputs (every terrain is
met, the heightfields answer differently) are checked from the oracle alone in tests/test_world_batch_terrains_host.py."""
import numpy as np
import pytest

import mgf_amd
from mgf_amd import scenes
from tests import batch_observe_cases as OC
from tests import batch_terrain_cases as TC
from tests import contact_corpus as CC
from tests.util import bits_equal, compare_constraints, oracle_world

pytestmark = pytest.mark.gpu

STATE = ("x", "q", "v", "omega", "delta")
COUNTS = ("n_constraints", "n_terrain_constraints", "n_pair_candidates", "n_refits")
INV = mgf_amd._capi.ERR_INVALID
BODIES, TERRAIN, ALL = mgf_amd._capi.QUERY_BODIES, mgf_amd._capi.QUERY_TERRAIN, mgf_amd._capi.QUERY_ALL


@pytest.fixture(scope="module")
def ctx():
    c = mgf_amd.Context(0)
    yield c
    c.close()


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_state(got, want, what):
    for f in STATE:
        assert bits_equal(got[f], want[f]), f"{what}: {f} differs"


def _same_world(a, ka, b, kb, what):
    _same_state(a.state(ka), b.state(kb), what)
    compare_constraints(a.constraints(ka), b.constraints(kb), check_impulse=True)


def _mesh(ctx, t, pos=None):
    m = mgf_amd.Mesh(ctx)
    m.build(t["verts"], t["faces"])
    m.set_pos(t["pos"] if pos is None else pos)
    return m


def _step_lone(lone, dt, iters, n=1):
    for w in lone:
        if len(w):
            w.step_many(dt, iters, n)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(ctx):
    """the six worlds of TC.mixed_scenes in one batch, free running beside one oracle world each: every tick the state bits and the four
    counts, at TC.LIST_TICKS the lists with impulses; then the lone worlds brought to the same tick (tests 1, 2, 5 and 6 share all this)"""
    scs = TC.mixed_scenes()
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    ows = [oracle_world(sc) for sc in scs]
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    seen_t = [0] * len(scs)
    for tick in range(1, TC.TICKS + 1):
        st = b.step(dt, iters)
        for k, ow in enumerate(ows):
            ost = ow.step(dt, iters)
            what = f"world {k} tick {tick}"
            assert st[k].n_bodies == len(scs[k]["comps"]) and st[k].iters == iters
            for f in COUNTS:
                assert getattr(st[k], f) == getattr(ost, f), f"{what}: {f} = {getattr(st[k], f)}, the oracle has {getattr(ost, f)}"
            _same_state(b.state(k), ow.state(), what)
            if tick in TC.LIST_TICKS:
                compare_constraints(b.constraints(k), ow.constraints(), check_impulse=True)
            seen_t[k] = max(seen_t[k], int(ost.n_terrain_constraints))
    lone = [mgf_amd.World.from_scene(ctx, sc) for sc in scs]
    _step_lone(lone, dt, iters, TC.TICKS)
    return dict(scs=scs, b=b, ows=ows, lone=lone, seen_t=seen_t, dt=dt, iters=iters)


def test_mixed_terrains_against_the_oracle_free_running(mixed):
    scs, b, lone = mixed["scs"], mixed["b"], mixed["lone"]
    print("most terrain constraints per world:", mixed["seen_t"])
    assert all((t > 0) == (sc["terrain"] is not None and len(sc["comps"]) > 0) for t, sc in zip(mixed["seen_t"], scs)), mixed["seen_t"]
    assert b.counter("launches_per_tick") == 6 and b.terrain_count() == 3
    rng = np.random.default_rng(8)
    whole = b.body_contacts()
    at = 0
    for k, sc in enumerate(scs):
        n = len(sc["comps"])
        if n:
            _same_state(b.state(k), lone[k].state(), f"world {k} against the lone world")
            cons = lone[k].constraints()
            compare_constraints(b.constraints(k), cons, check_impulse=True)
            want = OC.fold(cons, n)
            assert same_bytes(b.body_contacts(k), want) and same_bytes(whole[at:at + n], want), f"world {k}: contact summaries"
            if sc["terrain"] is not None:
                assert want["n_terrain"].sum() > 0, k
            cen = TC.centres_of(b.colliders(k))
            boxes = np.concatenate([cen[rng.integers(0, n, 6)] + rng.normal(0, 0.4, (6, 3)), rng.uniform(0.2, 1.5, (6, 1)) * np.ones((1, 3))], axis=1).astype(np.float32)
            off, vals = b.overlap_boxes(k, boxes)
            loff, lvals = lone[k].overlap_boxes(boxes)
            assert np.array_equal(off, loff) and np.array_equal(vals, lvals) and len(vals) > 0, f"world {k}: box overlaps"
        at += n


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_placement_does_not_matter(ctx, mixed):
    scs, b, dt, iters = mixed["scs"], mixed["b"], mixed["dt"], mixed["iters"]
    K = len(scs)
    # the worlds in reverse order, the table built by hand in another order (box, second heightfield, first heightfield) with an entry
    # nobody uses in front and the shared geometry added at the twin's raised position
    rb = mgf_amd.WorldBatch.from_scenes(ctx, [dict(sc, terrain=None) for sc in scs[::-1]])
    unused = rb.add_terrain(_mesh(ctx, scenes.sphere_pile(2, 2, 2)["terrain"]))
    box, hf_b, hf_a = (rb.add_terrain(_mesh(ctx, scs[k]["terrain"])) for k in (2, 1, 3))
    assert (unused, box, hf_b, hf_a) == (0, 1, 2, 3) and rb.terrain_count() == 4
    ids = {0: hf_a, 1: hf_b, 2: box, 3: hf_a, 4: -1, 5: box}
    for k in range(K):   # (one call a world, and world 0 named twice in its call: the last assignment holds)
        pos = scs[k]["terrain"]["pos"] if scs[k]["terrain"] is not None else (0.0, 0.0, 0.0)
        rb.set_world_terrain([K - 1 - k, K - 1 - k], [unused, ids[k]], [(9.0, 9.0, 9.0), pos])
    rb.step(dt, iters, TC.TICKS)
    for k in range(K):
        _same_world(rb, K - 1 - k, b, k, f"world {k} in the batch built in reverse")
    assert rb.counter("launches_per_tick") == 6


def test_more_worlds_than_compute_units_cycling_over_three_terrains(ctx):
    small = TC.small_scenes()
    dt, iters = float(small[0]["dt"]), small[0]["iters"]
    K = 300
    three = mgf_amd.WorldBatch.from_scenes(ctx, small, own_terrain=True)
    many = mgf_amd.WorldBatch.from_scenes(ctx, [small[k % 3] for k in range(K)], own_terrain=True)
    assert three.terrain_count() == many.terrain_count() == 2
    st3, stm = three.step(dt, iters, 30), many.step(dt, iters, 30)
    assert all(max(st3[t * 3 + k].n_terrain_constraints for t in range(30)) > 0 for k in range(3))
    whole, ref = many.state(), [three.state(k) for k in range(3)]
    at = 0
    for k in range(K):
        n = len(small[k % 3]["comps"])
        _same_state({f: whole[f][at:at + n] for f in STATE}, ref[k % 3], f"copy {k}")
        assert stm[29 * K + k].as_dict() == st3[29 * 3 + k % 3].as_dict(), k
        if k % 37 == 0 or k == K - 1:
            compare_constraints(many.constraints(k), three.constraints(k % 3), check_impulse=True)
        at += n
    # the queries' launches depend neither on the worlds nor on the queries (6 worlds: test 5)
    p = np.tile(np.float32([0.2, 20.0, 0.1]), (4096, 1))
    d = np.tile(np.float32([0.0, -1.0, 0.0]), (4096, 1))
    casts = np.zeros(4096, mgf_amd.MOVING_DTYPE)
    casts["p"], casts["r"], casts["delta"] = p, 0.3, (0.0, -25.0, 0.0)
    world = (np.arange(4096) % K).astype(np.int32)
    many.colliders(0)   # (the colliders gathered behind the step: not a launch of the calls counted below)
    three.colliders(0)
    counts = []
    for n in (1, 4096):
        r = many.raycast(world[:n], p[:n], d[:n])
        lr = many.counter("query_launches")
        s = many.sweep(world[:n], casts[:n])
        counts.append((lr, many.counter("query_launches")))
        assert np.all(r["kind"] >= 0) and np.all(s["kind"] >= 0)
        assert same_bytes(r[:3], three.raycast(world[:3] % 3, p[:3], d[:3])[:n]) and same_bytes(s[:3], three.sweep(world[:3] % 3, casts[:3])[:n])
    counts.append((None, None))
    three.raycast(world[:5] % 3, p[:5], d[:5])
    lr = three.counter("query_launches")
    three.sweep(world[:5] % 3, casts[:5])
    counts[2] = (lr, three.counter("query_launches"))
    assert counts[0] == counts[1] == counts[2] and counts[0][0] == 1 and counts[0][1] == 2, counts


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_reassignment_between_ticks(ctx):
    scs = TC.mixed_scenes()[:4]
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    T0, T1 = 15, 25
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    ref = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    lone = [mgf_amd.World.from_scene(ctx, sc) for sc in scs]
    ows = [oracle_world(sc) for sc in scs]
    b.step(dt, iters, T0)
    ref.step(dt, iters, T0)
    _step_lone(lone, dt, iters, T0)
    for ow in ows:
        for _ in range(T0):
            ow.step(dt, iters)
    # world 0 to the other heightfield; world 1 keeps its mesh at a new position; world 2 loses its box; world 3 stays as it is
    tb = scs[1]["terrain"]
    moved = np.float32([0.05, 0.15, -0.1])
    assert b.terrain_count() == 3
    b.set_world_terrain([0, 1, 2], [1, 1, -1], [tb["pos"], moved, (0.0, 0.0, 0.0)])
    keep = [_mesh(ctx, tb), _mesh(ctx, tb, moved)]
    lone[0].set_terrain(keep[0])
    lone[1].set_terrain(keep[1])
    lone[2].set_terrain(None)
    ows[0].set_terrain(tb["verts"], tb["faces"], tb["pos"])
    ows[1].set_terrain(tb["verts"], tb["faces"], moved)
    ows[2].set_terrain(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), (0.0, 0.0, 0.0))
    seen = [0, 0, 0, 0]
    for tick in range(T0 + 1, T0 + T1 + 1):
        st = b.step(dt, iters)
        _step_lone(lone, dt, iters)
        for k, ow in enumerate(ows):
            ost = ow.step(dt, iters)
            for f in COUNTS:
                assert getattr(st[k], f) == getattr(ost, f), (k, tick, f)
            _same_state(b.state(k), ow.state(), f"world {k} tick {tick}")
            seen[k] = max(seen[k], int(ost.n_terrain_constraints))
        if tick in (T0 + 1, T0 + 2, T0 + 10, T0 + T1):
            for k in range(4):
                compare_constraints(b.constraints(k), ows[k].constraints(), check_impulse=True)
                _same_state(b.state(k), lone[k].state(), f"world {k} tick {tick} against the lone world")
                compare_constraints(b.constraints(k), lone[k].constraints(), check_impulse=True)
    assert seen[0] > 0 and seen[1] > 0 and seen[2] == 0 and seen[3] > 0, seen
    ref.step(dt, iters, T1)
    _same_world(b, 3, ref, 3, "the world nothing was re-assigned in")
    for k in (0, 1, 2):
        assert not bits_equal(b.state(k)["x"], ref.state(k)["x"]), f"world {k}: the re-assignment changed nothing"


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rung", CC.WORLD_RUNGS, ids=[f"rung{r}" for r in CC.WORLD_RUNGS])
def test_the_contact_corpus_with_a_mesh_per_world(ctx, rung):
    K = 16
    allp = CC.plant(CC.base_cases(CC.PAIR_TYPES), rung)
    tris = CC.plant(CC.base_cases(CC.TRI_TYPES, per_family=8), rung)
    worlds = [CC.with_mesh(CC.pair_world(allp[k::K]), tris[k::K]) for k in range(K)]
    b = mgf_amd.WorldBatch(ctx, K)
    order = [(5 * k + 3) % K for k in range(K)]   # the table in an order of its own
    ids = {k: b.add_terrain(_mesh(ctx, worlds[k]["mesh"])) for k in order}
    assert b.terrain_count() == K and sorted(ids.values()) == list(range(K))
    b.set_world_terrain(np.arange(K), [ids[k] for k in range(K)])
    for k, sc in enumerate(worlds):
        assert len(sc["comps"]) <= mgf_amd.BATCH_MAX_BODIES
        b.add_bodies(k, sc["comps"], 1.0, 0.3, 0.6, (0.0, 0.0, 0.0))
        b.write_state(k, v=sc["delta"])
    st = b.step(1.0, CC.ITERS)
    total = terrain = 0
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
        assert ost.n_constraints > 100 and ost.n_terrain_constraints > 0, (what, ost.n_constraints, ost.n_terrain_constraints)
        total += int(ost.n_constraints)
        terrain += int(ost.n_terrain_constraints)
    print(f"rung {rung}: {total} constraints ({terrain} against the meshes) in {K} worlds, capacity_retries {b.counter('capacity_retries')}")


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_queries_see_the_terrain_of_their_world(mixed):
    scs, b, lone, ows = mixed["scs"], mixed["b"], mixed["lone"], mixed["ows"]
    K = len(scs)
    cols = [ow.colliders()[0] for ow in ows]
    for k in range(K):
        got = b.colliders(k)
        assert all(np.array_equal(got[f], cols[k][f]) for f in ("tag", "p", "d", "r")), f"world {k}: colliders"   # so the rays are the host check's
    cen = [TC.centres_of(c) for c in cols]
    rays = TC.mixed_rays(cen)
    world, p, d, dt, ign = rays["world"], rays["p"], rays["d"], rays["dt"], rays["ignore"]
    launches = set()
    for kinds in (ALL, BODIES, TERRAIN):
        got = b.raycast(world, p, d, dt, ignore=ign, kinds=kinds)
        launches.add(b.counter("query_launches"))
        for k in range(K):
            sel = world == k
            assert same_bytes(got[sel], lone[k].raycast(p[sel], d[sel], dt[sel], ignore=ign[sel], kinds=kinds)), f"world {k} kinds {kinds}: rays"
            seen = set(got[sel]["kind"].tolist())
            if kinds == ALL and scs[k]["terrain"] is not None and len(scs[k]["comps"]):
                assert seen == {-1, 0, 1}, (k, seen)
            if kinds == TERRAIN and scs[k]["terrain"] is None:
                assert seen == {-1}, (k, seen)   # a ray into the world without terrain meets nothing
        if kinds == TERRAIN:
            probes = {k: got[(world == k) & (rays["probe"] >= 0)][np.argsort(rays["probe"][(world == k) & (rays["probe"] >= 0)])] for k in range(K)}
            for x, y in (TC.HEIGHTFIELDS, TC.TWINS):
                both = (probes[x]["kind"] == 1) & (probes[y]["kind"] == 1)
                assert np.any(both & ((probes[x]["t"] != probes[y]["t"]) | (probes[x]["index"] != probes[y]["index"]))), (x, y)
    one = b.raycast(world[:1], p[:1], d[:1], dt[:1], ignore=ign[:1])
    launches.add(b.counter("query_launches"))
    assert launches == {1}, launches
    cw, casts = TC.mixed_casts(cen)
    assert np.any((casts["tag"] == 1) & np.all(casts["delta"] == 0, axis=1)) and np.any((casts["tag"] == 0) & np.all(casts["delta"] == 0, axis=1))
    launches = {}
    for kinds in (ALL, BODIES, TERRAIN):
        got = b.sweep(cw, casts, kinds=kinds)
        launches[kinds] = b.counter("query_launches")
        for k in range(K):
            sel = cw == k
            assert same_bytes(got[sel], lone[k].sweep(casts[sel], kinds=kinds)), f"world {k} kinds {kinds}: sweeps"
            if scs[k]["terrain"] is None:
                assert kinds == TERRAIN and np.all(got[sel]["kind"] == -1) or kinds != TERRAIN and np.all(got[sel]["kind"] != 1), k
        if kinds == TERRAIN:
            assert all(np.any(got[cw == k]["kind"] == 1) for k in range(K) if scs[k]["terrain"] is not None)
        if kinds == ALL:
            assert np.any(got["kind"] == 1)
        if kinds != TERRAIN:
            assert all(np.any(got[cw == k]["kind"] == 0) for k in range(K) if len(scs[k]["comps"])), kinds
    b.sweep(cw[:1], casts[:1])
    assert launches == {ALL: 2, BODIES: 1, TERRAIN: 2} and b.counter("query_launches") == 2, launches
    # a query touches nothing of the tick: the worlds go on as the oracle's do
    b2 = mixed["b"]
    st = b2.step(mixed["dt"], mixed["iters"])
    _step_lone(lone, mixed["dt"], mixed["iters"])
    for k, ow in enumerate(ows):
        ow.step(mixed["dt"], mixed["iters"])
        _same_state(b2.state(k), ow.state(), f"world {k} a tick behind the queries")


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_capacity_reruns_with_differing_terrains(ctx):
    scs = TC.mixed_scenes()
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    b.set_option("cons_per_body", 1)
    ref = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    st, rst = b.step(dt, iters, TC.TICKS), ref.step(dt, iters, TC.TICKS)
    assert b.counter("capacity_retries") > 0
    assert [s.as_dict() for s in st] == [s.as_dict() for s in rst]
    ows, _ = TC.run_oracles(scs, TC.TICKS)
    for k, ow in enumerate(ows):
        _same_world(b, k, ref, k, f"world {k}")
        _same_state(b.state(k), ow.state(), f"world {k} against the oracle")
        compare_constraints(b.constraints(k), ow.constraints(), check_impulse=True)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_old_entry_point_is_the_new_one(ctx):
    big = scenes.sphere_pile(4, 6, 4, seed=5)
    scs = [dict(sc, terrain=big["terrain"]) for sc in (big, scenes.sphere_pile(1, 1, 1))]
    dt, iters = float(big["dt"]), big["iters"]
    old = mgf_amd.WorldBatch.from_scenes(ctx, scs)
    new = mgf_amd.WorldBatch.from_scenes(ctx, [dict(sc, terrain=None) for sc in scs])
    assert old.terrain_count() == 1 and new.terrain_count() == 0
    m = _mesh(ctx, big["terrain"])
    assert new.add_terrain(m) == 0
    new.set_world_terrain([0, 1], 0)
    so, sn = old.step(dt, iters, 60), new.step(dt, iters, 60)
    assert [s.as_dict() for s in so] == [s.as_dict() for s in sn]
    assert max(s.n_terrain_constraints for s in so[0::2]) > 0 and max(s.n_terrain_constraints for s in so[1::2]) > 0
    for k in range(2):
        _same_world(new, k, old, k, f"world {k}")
    # set_terrain(None) behind add_terrain: an empty table, no world has terrain
    new.add_terrain(m)
    assert new.terrain_count() == 2
    new.set_terrain(None)
    assert new.terrain_count() == 0
    st = new.step(dt, iters, 30)
    assert all(s.n_terrain_constraints == 0 for s in st)
    assert all(np.all(new.constraints(k)["b"] >= 0) for k in range(2))
    assert new.state(1)["x"][0, 1] < -0.5   # the lone sphere has fallen through where the floor was
    # and set_terrain(m) behind that is the shared mesh again: entry 0, every world
    new.set_terrain(m)
    assert new.terrain_count() == 1 and new.add_terrain(m) == 1


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_that_need_a_real_handle(ctx):
    scs = TC.small_scenes()
    dt, iters = float(scs[0]["dt"]), scs[0]["iters"]
    b = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    ref = mgf_amd.WorldBatch.from_scenes(ctx, scs, own_terrain=True)
    b.step(dt, iters, 5)
    ref.step(dt, iters, 5)
    n = b.terrain_count()
    assert n == 2
    for world, terrain, word in (([0, 3], [-1, -1], "world index"), ([0, 1], [-1, n], "terrain id"), ([0, 1], [-1, -2], "terrain id"),
                                 ([1, 0, 1 << 20], [-1, -1, 0], "world index")):
        with pytest.raises(mgf_amd.MgfError) as e:
            b.set_world_terrain(world, terrain, (5.0, 5.0, 5.0))   # (the first assignment of each call is a valid one: it must not be applied)
        assert e.value.status == INV and word in str(e.value), (world, terrain, str(e.value))
    assert b.terrain_count() == n
    st, rst = b.step(dt, iters, 10), ref.step(dt, iters, 10)
    assert [s.as_dict() for s in st] == [s.as_dict() for s in rst]
    assert max(s.n_terrain_constraints for s in st[0::3]) > 0
    for k in range(3):
        _same_world(b, k, ref, k, f"world {k} behind the refused calls")
