"""k_contacts_rows in two (option contacts_split): the numbering ahead of the solver's table kernels (k_contacts_rows_index), the partner contacts'
records beside them as foreign blocks of k_flow6_links' launch (k_flow6_links_records) - or in a launch of their own where no tables are built inside
the collide phase.  Every case: the split tick against the unsplit one (contacts_split = 0) and, over its first ticks, against the oracle, bit for bit;
the counters say which path ran; no record job is left pending."""
import numpy as np
import pytest

from tests.util import compare_constraints, oracle_world, values_equal

pytestmark = pytest.mark.gpu

FUSED, ALONE = "contacts_split_fused", "contacts_split_standalone"


@pytest.fixture(scope="module")
def ctx():
    import mgf_amd
    c = mgf_amd.Context(0)
    yield c
    c.close()


def dense_scene(nx, pitch, seed=3):
    """(tests/test_gpu_contacts_dense.py's lattice of pressed spheres)"""
    from mgf_amd import scenes
    rng = np.random.default_rng(seed)
    i, j, k = np.meshgrid(np.arange(nx), np.arange(nx), np.arange(nx), indexing="ij")
    c = (np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1) * pitch).astype(np.float32)
    c += rng.uniform(-0.03, 0.03, c.shape).astype(np.float32)
    c[:, 0] -= np.float32(0.5 * nx * pitch); c[:, 2] -= np.float32(0.5 * nx * pitch); c[:, 1] += np.float32(0.5)
    c = c[rng.permutation(len(c))]
    v0 = rng.uniform(-0.5, 0.5, c.shape).astype(np.float32)
    terrain = scenes.box_terrain(nx * pitch + 4.0, nx * pitch + 6.0, (0.0, 0.0, 0.0))
    return scenes._scene(f"dense_{nx}", scenes._spheres(c, 0.5), terrain, v0=v0, iters=4)


def _world(ctx, scene, split, opts):
    import mgf_amd
    w = mgf_amd.World.from_scene(ctx, scene)
    for k, v in opts.items():
        w.set_option(k, v)
    w.set_option("contacts_split", split)
    return w


def _same(a, b, what, oracle=False):
    compare_constraints(a.constraints(), b.constraints(), check_impulse=not oracle)
    sa, sb = a.state(), b.state()
    for k in ("x", "q", "v", "omega"):
        assert values_equal(sa[k], sb[k]), (what, k)


def _paths(w, split=True):
    """-> ticks by path.  Nothing is pending outside a collide phase; every tick that ended on the rows' front ends (k_contacts_rows' callers) took one
    of the two paths - a tick that is run again takes the candidate lists (its k_integrate's rows are stale), which the split does not touch."""
    assert w.counter("contacts_records_pending") == 0
    fused, alone = w.counter(FUSED), w.counter(ALONE)
    assert fused + alone == (w.counter("fused_contacts_ticks") + w.counter("front_rows_ticks") if split else 0), (fused, alone)
    return fused, alone


def _run(ctx, scene, ticks, opts, every, oracle_ticks, split=1):
    """`ticks` ticks of the split world and the unsplit one, step_many `every` at a time, compared behind each batch - and with the oracle over the
    first `oracle_ticks`.  -> the split world, the unsplit world"""
    dt, it = float(scene["dt"]), scene["iters"]
    a, b = _world(ctx, scene, split, opts), _world(ctx, scene, 0, opts)
    ow = oracle_world(scene)
    for t0 in range(0, ticks, every):
        na = [int(s.n_constraints) for s in a.step_many(dt, it, every)]
        nb = [int(s.n_constraints) for s in b.step_many(dt, it, every)]
        assert na == nb, t0
        _same(a, b, t0 + every)
        if t0 + every <= oracle_ticks:
            for _ in range(every):
                ow.step(dt, it)
            _same(a, ow, ("oracle", t0 + every), oracle=True)
    assert _paths(b, False) == (0, 0)
    return a, b


@pytest.mark.parametrize("pitch", [0.62, 0.68])
def test_dense_lattice_long_rows_and_second_windows(ctx, pitch):
    """rows of 13+ entries (cs_list_row's long form) and blocks past kCsEntCap = 1536 entries (the second window).
    At a pitch of 0.62 a body's fat box meets more than kRowCap = 48 others: the pair search's rows overflow, every tick is run again on the exact
    two-pass candidate lists and neither form of k_contacts_rows writes its records (two_pass_ticks == 3) - what is compared there is that the split
    launches, which return at the tick's fail word, leave nothing behind.  At 0.68 the second lattice neighbours (1.36 apart) stay out of the
    boxes, the first eighteen (0.68 and 0.96 apart) touch: nine contacts per body as `a` on average, blocks of two and three windows - with the
    global solver (mode 1), so that no tick is run again for the block-local solver's tables and the records come from the launch of their own;
    the first tick outgrows a new world's constraint capacity and is run again on the candidate lists."""
    sc = dense_scene(16, pitch)
    dt, it = float(sc["dt"]), sc["iters"]
    opts = {"solver_mode": 1} if pitch == 0.68 else {}
    ticks = 4 if pitch == 0.68 else 3
    a, b, ow = _world(ctx, sc, 1, opts), _world(ctx, sc, 0, opts), oracle_world(sc)
    for tick in range(ticks):
        sa, sb, so = a.step(dt, it), b.step(dt, it), ow.step(dt, it)
        assert sa.n_constraints == sb.n_constraints == so.n_constraints, tick
        co = ow.constraints()
        if tick == 0:
            per_a = np.bincount(co["a"][co["b"] >= 0], minlength=len(a))
            assert per_a.max() > 12 and len(co) > 6 * len(a), (per_a.max(), len(co))
            if pitch == 0.68:  # (blocks of 256 bodies of the caller's order past one window, and past two)
                per_block = per_a.reshape(-1, 256).sum(axis=1)
                assert per_block.max() > 2 * 1536 and (per_block > 1536).sum() >= 4, per_block
        _same(a, b, tick)
        _same(a, ow, ("oracle", tick), oracle=True)
    fused, alone = _paths(a)
    print("dense lattice", pitch, ": fused", fused, "standalone", alone, {k: a.counter(k) for k in ("flow6_fallbacks", "flow6_skipped", "fused_contacts_ticks", "two_pass_ticks", "capacity_retries", "row_overflows")})
    assert _paths(b, False) == (0, 0)
    if pitch == 0.62:
        assert a.counter("two_pass_ticks") == 3 and (fused, alone) == (0, 0)
    else:
        assert a.counter("two_pass_ticks") == 0 and fused == 0 and alone >= ticks - 1, (fused, alone)


@pytest.mark.parametrize("mode", [6, 1])
def test_sphere_pile_step_many_and_a_clone(ctx, mode):
    """1 728 bodies: a tail block of the bodies' launch; seven solver blocks and channels between them.  Mode 6: the records ride in the links launch;
    mode 1: no tables, a launch of their own.  A clone taken at tick 20 carries on identically."""
    from mgf_amd import scenes
    sc = scenes.sphere_pile(12, 12, 12)
    dt, it = float(sc["dt"]), sc["iters"]
    opts = {"flow5_block": 256, "solver_mode": mode}
    a, b = _run(ctx, sc, 20, opts, 10, 10)
    if mode == 6:
        assert a.counter("flow5_blocks") == 7
    c = a.clone()
    assert c.counter("contacts_records_pending") == 0
    for t0 in (20, 30):
        for w in (a, b, c):
            w.step_many(dt, it, 10)
        _same(a, b, t0 + 10)
        _same(c, b, ("clone", t0 + 10))
    assert a.stats.n_constraints > 3000
    want = (40, 0) if mode == 6 else (0, 40)
    assert _paths(a) == want and a.counter("flow6_fallbacks") == 0, (_paths(a), a.counter("flow6_fallbacks"))
    fc, ac = _paths(c)
    assert (fc > 0) == (mode == 6) and (ac > 0) == (mode == 1)


def test_capsules_over_a_face_grid(ctx):
    """k_contacts_rows_index<false> with the terrain constraints a lane per slot (t_blocks > 0), the records by k_flow6_links_records<false>"""
    from mgf_amd import scenes
    sc = scenes.capsule_field(8, 6, 8, quads=12, pitch=1.6)
    a, b = _run(ctx, sc, 60, {}, 10, 10)
    assert a.counter("terrain_grid") == 1 and a.counter("front_rows_ticks") == 60 and a.stats.n_terrain_constraints > 0
    assert a.stats.n_constraints > a.stats.n_terrain_constraints
    assert _paths(a) == (60, 0) and a.counter("flow6_fallbacks") == 0, (_paths(a), a.counter("flow6_fallbacks"))


def test_empty_ticks_through_the_first_contact(ctx):
    """ticks without a constraint (record blocks that all leave at once; the links launch's ticket counts link blocks only and must re-arm)"""
    from mgf_amd import scenes
    sc = scenes.balls_demo(4)
    dt, it = float(sc["dt"]), sc["iters"]
    a, b, ow = _world(ctx, sc, 1, {}), _world(ctx, sc, 0, {}), oracle_world(sc)
    empty = ticks = 0
    while ticks < 400:
        na = [int(s.n_constraints) for s in a.step_many(dt, it, 10)]
        nb = [int(s.n_constraints) for s in b.step_many(dt, it, 10)]
        no = [int(ow.step(dt, it).n_constraints) for _ in range(10)]
        assert na == nb == no, ticks
        ticks += 10
        _same(a, b, ticks)
        _same(a, ow, ("oracle", ticks), oracle=True)
        empty += sum(1 for c in na if c == 0)
        if na[0] > 0:  # (a whole batch behind the first contact)
            break
    assert empty >= 10 and na[-1] > 0, (empty, na)
    assert _paths(a) == (ticks, 0) and a.counter("flow6_runs") >= ticks - empty, (_paths(a), ticks, empty)


def test_a_collide_phase_run_again_for_capacity(ctx):
    from mgf_amd import scenes
    sc = scenes.sphere_pile(10, 10, 10)
    dt, it = float(sc["dt"]), sc["iters"]
    a, b, ow = _world(ctx, sc, 1, {}), _world(ctx, sc, 0, {}), oracle_world(sc)
    for step in range(12):
        if step % 3 == 0:
            a.set_option("list_capacity", 7 + step)  # far too small once contacts exist
        sa, sb, so = a.step(dt, it), b.step(dt, it), ow.step(dt, it)
        assert sa.n_constraints == sb.n_constraints == so.n_constraints
        _same(a, b, step)
        _same(a, ow, ("oracle", step), oracle=True)
    assert sa.n_constraints > 1000 and a.counter("capacity_retries") >= 3
    # (four of the twelve ticks were run again: a re-run's k_integrate rows are stale, it takes the candidate lists - k_setup_pairs writes its records)
    assert _paths(a) == (8, 0) and a.counter("fused_contacts_ticks") == 8, _paths(a)


def test_a_flow6_failure_and_its_re_run(ctx):
    from mgf_amd import scenes
    sc = scenes.sphere_pile(10, 10, 10)
    dt, it = float(sc["dt"]), sc["iters"]
    a, b, ow = _world(ctx, sc, 1, {}), _world(ctx, sc, 0, {}), oracle_world(sc)
    a.step_many(dt, it, 6); b.step_many(dt, it, 6)
    for _ in range(6):
        ow.step(dt, it)
    assert _paths(a) == (6, 0)
    a.set_option("flow6_test_cap", 40); b.set_option("flow6_test_cap", 40)
    for t0 in (6, 12):
        a.step_many(dt, it, 6); b.step_many(dt, it, 6)
        for _ in range(6):
            ow.step(dt, it)
        _same(a, b, t0 + 6)
        _same(a, ow, ("oracle", t0 + 6), oracle=True)
    # (a tick whose tables did not fit is run again from the collide phase with the global solver - on the candidate lists: its k_integrate's rows are
    # stale - so its records are k_setup_pairs'; the first attempt's record blocks left with the tick's fail word or were overwritten)
    assert _paths(a) == (6, 0) and a.counter("flow6_fallbacks") >= 10, (_paths(a), a.counter("flow6_fallbacks"))


@pytest.mark.parametrize("dims", [(1, 1, 1), (5, 5, 8)])
def test_tiny_worlds(ctx, dims):
    from mgf_amd import scenes
    sc = scenes.sphere_pile(*dims)
    a, b = _run(ctx, sc, 10, {}, 5, 10)
    assert a.stats.n_constraints > 0
    fused, alone = _paths(a)
    assert fused + alone == 10 and alone == a.counter("flow6_fallbacks"), (fused, alone)
