"""The solver's block tables inside the numbering launch (option tables_fused: k_contacts_rows_index_tables - a ticket per solver block of a re-sorted
store, the block's binfo / bref / foreign bodies / rows written from what the numbering holds in LDS; no k_flow6_blocks launch).  Every case: the fused
tick against the tick with the separate launch (tables_fused = 0), bit for bit - constraints with impulses, x, q, v, omega, the constraint count of every
tick - and, over its first ticks, against the oracle; the counter tables_fused_ticks says which path ran (a tick that is run again takes the candidate
lists and counts in neither).  Small worlds are not re-sorted on their own: the fused cases set resort_every."""
import numpy as np
import pytest

from tests.test_gpu_contacts_split import dense_scene
from tests.util import compare_constraints, oracle_world, values_equal

pytestmark = pytest.mark.gpu

TABLES = "tables_fused_ticks"
RESORT = {"resort_every": 8}


@pytest.fixture(scope="module")
def ctx():
    import mgf_amd
    c = mgf_amd.Context(0)
    yield c
    c.close()


def _world(ctx, scene, fused, opts=None):
    import mgf_amd
    w = mgf_amd.World.from_scene(ctx, scene)
    for k, v in (opts or {}).items():
        w.set_option(k, v)
    w.set_option("tables_fused", fused)
    return w


def _same(a, b, what, oracle=False):
    compare_constraints(a.constraints(), b.constraints(), check_impulse=not oracle)
    sa, sb = a.state(), b.state()
    for k in ("x", "q", "v", "omega"):
        assert values_equal(sa[k], sb[k]), (what, k)


def _run(ctx, scene, ticks, opts, every, oracle_ticks):
    """`ticks` ticks of the fused world and the one with the k_flow6_blocks launch, step_many `every` at a time, compared behind each batch - and with
    the oracle over the first `oracle_ticks`.  -> the fused world, the other"""
    dt, it = float(scene["dt"]), scene["iters"]
    a, b = _world(ctx, scene, 1, opts), _world(ctx, scene, 0, opts)
    ow = oracle_world(scene) if oracle_ticks else None
    for t0 in range(0, ticks, every):
        na = [int(s.n_constraints) for s in a.step_many(dt, it, every)]
        nb = [int(s.n_constraints) for s in b.step_many(dt, it, every)]
        assert na == nb, (t0, na, nb)
        _same(a, b, t0 + every)
        if t0 + every <= oracle_ticks:
            for _ in range(every):
                ow.step(dt, it)
            _same(a, ow, ("oracle", t0 + every), oracle=True)
    assert b.counter(TABLES) == 0
    print({k: a.counter(k) for k in (TABLES, "scan_fused_numbering_ticks", "store_resorts", "flow5_blocks", "capacity_retries", "flow6_fallbacks")})
    return a, b


def _fused_every_tick(a, ticks):
    """every tick but the world's first - which runs on the caller's order: the first re-sort takes the first tick's cell sort - built its tables in
    the numbering launch, on a re-sorted store, with the block-local solver"""
    assert a.counter("store_resorts") > 0
    assert a.counter(TABLES) == ticks - 1 and a.counter("scan_fused_numbering_ticks") >= ticks - 1, (a.counter(TABLES), a.counter("scan_fused_numbering_ticks"))
    # (... and that first tick, in blocks of 1 024 bodies of the caller's order, may meet more foreign bodies than a new world's guess: run again, once)
    assert a.counter("capacity_retries") <= 1 and a.counter("flow6_fallbacks") <= 1


def test_seven_blocks_of_256_links_across_faces_and_a_clone(ctx):
    """1 728 bodies in blocks of 256: seven tickets, the last block with 192 bodies (three groups of threads idle in every block); links across block
    faces and foreign bodies.  20 ticks through step_many, the first 10 against the oracle; a clone taken at tick 20 carries on identically."""
    from mgf_amd import scenes
    sc = scenes.sphere_pile(12, 12, 12)
    dt, it = float(sc["dt"]), sc["iters"]
    a, b = _run(ctx, sc, 20, dict(RESORT, flow5_block=256), 10, 10)
    assert a.counter("flow5_blocks") == 7 and a.stats.n_constraints > 3000
    _fused_every_tick(a, 20)
    c = a.clone()
    for t0 in (20, 30):
        for w in (a, b, c):
            w.step_many(dt, it, 10)
        _same(a, b, t0 + 10)
        _same(c, b, ("clone", t0 + 10))
    assert a.counter(TABLES) == 39 and c.counter(TABLES) == 20


def test_two_blocks_of_four_groups(ctx):
    """the same pile in blocks of 1 024: two tickets, the second block short (704 bodies) with an empty group - config 2's shape at its smallest"""
    from mgf_amd import scenes
    sc = scenes.sphere_pile(12, 12, 12)
    a, b = _run(ctx, sc, 20, dict(RESORT, flow5_block=1024), 10, 10)
    assert a.counter("flow5_blocks") == 2 and a.stats.n_constraints > 3000
    _fused_every_tick(a, 20)


def test_a_run_that_is_no_multiple_of_256(ctx):
    """blocks of 320 bodies: the second group of threads holds 64 bodies of the run, the run's first body is no multiple of 256"""
    from mgf_amd import scenes
    sc = scenes.sphere_pile(12, 12, 12)
    a, b = _run(ctx, sc, 20, dict(RESORT, flow5_block=320), 10, 10)
    assert a.counter("flow5_blocks") == 6 and a.stats.n_constraints > 3000
    _fused_every_tick(a, 20)


@pytest.mark.parametrize("dims", [(1, 1, 1), (5, 5, 8)])
def test_one_block_no_foreign_body(ctx, dims):
    from mgf_amd import scenes
    sc = scenes.sphere_pile(*dims)
    a, b = _run(ctx, sc, 10, RESORT, 5, 10)
    assert a.counter("flow5_blocks") == 1 and a.stats.n_constraints > 0
    _fused_every_tick(a, 10)


def test_a_group_past_one_window(ctx):
    """512 pressed spheres at a pitch of 0.68 (tests/test_gpu_contacts_split.py's lattice) in one block of 1 024, two groups of 256 bodies.  The first
    tick outgrows a new world's constraint capacity and is run again on the candidate lists.  The second builds its tables in the numbering launch
    with more than 2 x kCsEntCap = 3 072 partner contacts in the block: whatever the store's order, one of the two groups lists more than a window's
    worth - a second window, whose rows and brefs are written behind the first's.  (The spheres push each other apart: later ticks have fewer.)"""
    sc = dense_scene(8, 0.68)
    dt, it = float(sc["dt"]), sc["iters"]
    opts = dict(RESORT, flow5_block=1024)
    a, b, ow = _world(ctx, sc, 1, opts), _world(ctx, sc, 0, opts), oracle_world(sc)
    seen = []
    for tick in range(3):
        before = a.counter(TABLES)
        sa, sb, so = a.step(dt, it), b.step(dt, it), ow.step(dt, it)
        assert sa.n_constraints == sb.n_constraints == so.n_constraints, tick
        seen.append((a.counter(TABLES) - before, int((np.asarray(a.constraints()["b"]) >= 0).sum())))
        _same(a, b, tick)
        _same(a, ow, ("oracle", tick), oracle=True)
    print(seen, {k: a.counter(k) for k in ("scan_fused_numbering_ticks", "store_resorts", "capacity_retries", "flow6_fallbacks", "flow5_blocks")})
    assert a.counter("flow5_blocks") == 1 and a.counter("store_resorts") > 0 and b.counter(TABLES) == 0
    assert seen[1][0] == 1 and seen[1][1] > 2 * 1536, seen
    assert seen[0][0] == 0 and seen[2][0] == 1, seen


@pytest.mark.parametrize("opts", [{"resort_every": 0}, dict(RESORT, contacts_split=0)])
def test_the_separate_launch_stays(ctx, opts):
    """a store in the caller's order (blocks are runs of the tick's cell order, not of slots); the unsplit k_contacts_rows (no numbering launch)"""
    from mgf_amd import scenes
    sc = scenes.sphere_pile(12, 12, 12)
    a, b = _run(ctx, sc, 10, dict(opts, flow5_block=256), 5, 10)
    assert a.counter(TABLES) == 0 and a.counter("fused_contacts_ticks") == 10 and a.stats.n_constraints > 0


def test_a_capacity_between_two_blocks(ctx):
    """a constraint capacity that the first blocks' ids fit and the later ones' do not: the first blocks have written their tables when the closing
    block reports kFailConsCap, the others return early - the tick is run again on the candidate lists, with k_flow6_blocks, and counts in neither"""
    from mgf_amd import scenes
    sc = scenes.sphere_pile(12, 12, 12)
    dt, it = float(sc["dt"]), sc["iters"]
    opts = dict(RESORT, flow5_block=256)
    a, b, ow = _world(ctx, sc, 1, opts), _world(ctx, sc, 0, opts), oracle_world(sc)
    a.step_many(dt, it, 10); b.step_many(dt, it, 10)
    for _ in range(10):
        ow.step(dt, it)
    _same(a, b, 10)
    total = int(a.stats.n_constraints)
    assert total > 1000 and a.counter(TABLES) == 9 and a.counter("capacity_retries") == 0 and a.counter("store_resorts") > 0
    for step in range(3):
        a.set_option("list_capacity", total // 2)
        sa, sb, so = a.step(dt, it), b.step(dt, it), ow.step(dt, it)
        assert sa.n_constraints == sb.n_constraints == so.n_constraints
        _same(a, b, 11 + step)
        _same(a, ow, ("oracle", 11 + step), oracle=True)
    assert a.counter("capacity_retries") >= 3 and a.counter(TABLES) == 9 and a.counter("scan_fused_numbering_ticks") == 10


def test_a_flow6_failure_and_its_re_run(ctx):
    """flow6_test_cap = 40: the numbering launch raises fail bit 2 as k_flow6_blocks does; the tick is run again with the global solver"""
    from mgf_amd import scenes
    sc = scenes.sphere_pile(10, 10, 10)
    dt, it = float(sc["dt"]), sc["iters"]
    a, b, ow = _world(ctx, sc, 1, RESORT), _world(ctx, sc, 0, RESORT), oracle_world(sc)
    a.step_many(dt, it, 6); b.step_many(dt, it, 6)
    for _ in range(6):
        ow.step(dt, it)
    assert a.counter(TABLES) == 5 and a.counter("store_resorts") > 0
    a.set_option("flow6_test_cap", 40); b.set_option("flow6_test_cap", 40)
    for t0 in (6, 12):
        a.step_many(dt, it, 6); b.step_many(dt, it, 6)
        for _ in range(6):
            ow.step(dt, it)
        _same(a, b, t0 + 6)
        _same(a, ow, ("oracle", t0 + 6), oracle=True)
    assert a.counter(TABLES) == 5 and a.counter("flow6_fallbacks") >= 10, (a.counter(TABLES), a.counter("flow6_fallbacks"))
    assert b.counter(TABLES) == 0 and b.counter("flow6_fallbacks") == a.counter("flow6_fallbacks")


def test_capsules_keep_k_flow6_blocks(ctx):
    from mgf_amd import scenes
    sc = scenes.capsule_field(8, 6, 8, quads=12, pitch=1.6)
    a, b = _run(ctx, sc, 20, RESORT, 10, 10)
    assert a.counter("front_rows_ticks") == 20 and a.counter(TABLES) == 0 and a.stats.n_constraints > 0
