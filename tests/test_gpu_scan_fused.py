"""The constraint numbering inside k_contacts_rows_index's launch (option scan_fused, bit 1: k_contacts_rows_index_scan - ticketed runs of 1 024 bodies,
a status word per run, a look-back by the block's first wave; no k_scan<1> launch over p_cnt + tcn).  Every case: the fused tick against the tick with
the scan launch (scan_fused = 0), bit for bit - constraints, x, q, v, omega, the constraint count of every tick - and, where it is quick enough, against
the oracle; the counter says which path ran (a tick that is run again takes the candidate lists and counts in neither)."""
import pytest

from tests.util import compare_constraints, oracle_world, values_equal

pytestmark = pytest.mark.gpu

NUMBERED = "scan_fused_numbering_ticks"


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
    w.set_option("scan_fused", fused)
    return w


def _same(a, b, what, oracle=False):
    compare_constraints(a.constraints(), b.constraints(), check_impulse=not oracle)
    sa, sb = a.state(), b.state()
    for k in ("x", "q", "v", "omega"):
        assert values_equal(sa[k], sb[k]), (what, k)


def _numbered(w, fused=True):
    """-> the ticks numbered inside the index launch: every tick that ended on the spheres' rows (fused_contacts_ticks) with the option on, none without"""
    n = w.counter(NUMBERED)
    assert n == (w.counter("fused_contacts_ticks") if fused else 0), (n, w.counter("fused_contacts_ticks"))
    return n


def _run(ctx, scene, ticks, opts, every, oracle_ticks, fused=1):
    """`ticks` ticks of the fused world and the one with the scan launch, step_many `every` at a time, compared behind each batch - and with the oracle
    over the first `oracle_ticks`.  -> the fused world, the other"""
    dt, it = float(scene["dt"]), scene["iters"]
    a, b = _world(ctx, scene, fused, opts), _world(ctx, scene, 0, opts)
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
    assert _numbered(b, False) == 0
    return a, b


def test_sphere_pile_two_runs_a_tail_group_and_a_clone(ctx):
    """1 728 bodies: two runs (workgroups of four groups of 256 bodies), the second with a short group (192 bodies) and an empty one; base[n] by the
    closing block's first thread.  20 ticks through step_many, the first 10 against the oracle; a clone taken at tick 20 carries on identically."""
    from mgf_amd import scenes
    sc = scenes.sphere_pile(12, 12, 12)
    dt, it = float(sc["dt"]), sc["iters"]
    a, b = _run(ctx, sc, 20, {"flow5_block": 256}, 10, 10)
    assert a.counter("flow5_blocks") == 7 and a.stats.n_constraints > 3000
    assert (len(a) + a.counter("scan_fused_run") - 1) // a.counter("scan_fused_run") == 2
    assert _numbered(a) == 20 and a.counter("capacity_retries") == 0
    c = a.clone()
    for t0 in (20, 30):
        for w in (a, b, c):
            w.step_many(dt, it, 10)
        _same(a, b, t0 + 10)
        _same(c, b, ("clone", t0 + 10))
    assert _numbered(a) == 40 and _numbered(c) == 20


def test_more_runs_than_one_sweep_of_the_look_back(ctx):
    """65^3 = 274 625 bodies: 269 runs of 1 024, more than the 256 status words one sweep of the look-back reads - the runs behind the 256th take a second
    step (or stop at an inclusive prefix).  The smallest cube with more runs than the window.  Against scan_fused = 0 only: the oracle is too slow here."""
    from mgf_amd import scenes
    sc = scenes.sphere_pile(65, 65, 65)
    a, b = _run(ctx, sc, 10, {}, 5, 0)
    look, per_run = a.counter("scan_fused_look"), a.counter("scan_fused_run")
    runs = (len(a) + per_run - 1) // per_run
    assert runs > look and (64 ** 3 + per_run - 1) // per_run <= look, (runs, look)
    assert a.stats.n_constraints > len(a)  # (ten ticks into the fall: more than a contact per body)
    assert _numbered(a) + a.counter("capacity_retries") >= 10 and _numbered(a) >= 8, (_numbered(a), a.counter("capacity_retries"))


@pytest.mark.parametrize("dims", [(1, 1, 1), (5, 5, 8)])
def test_tiny_worlds(ctx, dims):
    """one run, short (groups without a body): run 0 publishes its inclusive prefix at once and is the closing block too"""
    from mgf_amd import scenes
    sc = scenes.sphere_pile(*dims)
    a, b = _run(ctx, sc, 10, {}, 5, 10)
    assert a.stats.n_constraints > 0 and _numbered(a) == 10


def test_empty_ticks_through_the_first_contact(ctx):
    """ticks without a constraint: every run's total is 0, the status words and the ticket are re-armed by the next tick's clearing launch all the same"""
    from mgf_amd import scenes
    sc = scenes.balls_demo(4)
    dt, it = float(sc["dt"]), sc["iters"]
    a, b, ow = _world(ctx, sc, 1), _world(ctx, sc, 0), oracle_world(sc)
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
    assert _numbered(a) == ticks and _numbered(b, False) == 0


def test_a_collide_phase_run_again_for_capacity(ctx):
    """list_capacity far too small: the closing block reports kFailConsCap with the whole count, the runs whose ids end inside the capacity have written
    theirs (nothing reads them; the re-run clears degb again) - the tick is run again on the candidate lists and agrees with the oracle"""
    from mgf_amd import scenes
    sc = scenes.sphere_pile(10, 10, 10)
    dt, it = float(sc["dt"]), sc["iters"]
    a, b, ow = _world(ctx, sc, 1), _world(ctx, sc, 0), oracle_world(sc)
    for step in range(12):
        if step % 3 == 0:
            a.set_option("list_capacity", 7 + step)  # far too small once contacts exist
        sa, sb, so = a.step(dt, it), b.step(dt, it), ow.step(dt, it)
        assert sa.n_constraints == sb.n_constraints == so.n_constraints
        _same(a, b, step)
        _same(a, ow, ("oracle", step), oracle=True)
    assert sa.n_constraints > 1000 and a.counter("capacity_retries") >= 3
    assert _numbered(a) == 8 and a.counter("fused_contacts_ticks") == 8  # (four of the twelve ticks were run again)
    assert _numbered(b, False) == 0


def test_a_capacity_between_two_runs(ctx):
    """1 728 bodies, two runs, and a constraint capacity that the first run's ids fit and the second run's do not: the first run has written its
    ab / rev / degb entries when the closing block reports kFailConsCap - the re-run must not see them"""
    from mgf_amd import scenes
    sc = scenes.sphere_pile(12, 12, 12)
    dt, it = float(sc["dt"]), sc["iters"]
    a, b, ow = _world(ctx, sc, 1), _world(ctx, sc, 0), oracle_world(sc)
    a.step_many(dt, it, 10); b.step_many(dt, it, 10)
    for _ in range(10):
        ow.step(dt, it)
    _same(a, b, 10)
    total = int(a.stats.n_constraints)
    first = int((a.constraints()["a"] < a.counter("scan_fused_run")).sum())  # (about the first run's share of the ids - the store's order need not be the caller's; the capacity below lies well between it and the total)
    assert 0 < first < total and _numbered(a) == 10 and a.counter("capacity_retries") == 0
    for step in range(3):
        a.set_option("list_capacity", (first + total) // 2)
        sa, sb, so = a.step(dt, it), b.step(dt, it), ow.step(dt, it)
        assert sa.n_constraints == sb.n_constraints == so.n_constraints
        _same(a, b, 11 + step)
        _same(a, ow, ("oracle", 11 + step), oracle=True)
    assert a.counter("capacity_retries") >= 3 and _numbered(a) == 10  # (every one of the three ticks was run again, on the candidate lists)


def test_a_flow6_failure_and_its_re_run(ctx):
    from mgf_amd import scenes
    sc = scenes.sphere_pile(10, 10, 10)
    dt, it = float(sc["dt"]), sc["iters"]
    a, b, ow = _world(ctx, sc, 1), _world(ctx, sc, 0), oracle_world(sc)
    a.step_many(dt, it, 6); b.step_many(dt, it, 6)
    for _ in range(6):
        ow.step(dt, it)
    assert _numbered(a) == 6
    a.set_option("flow6_test_cap", 40); b.set_option("flow6_test_cap", 40)
    for t0 in (6, 12):
        a.step_many(dt, it, 6); b.step_many(dt, it, 6)
        for _ in range(6):
            ow.step(dt, it)
        _same(a, b, t0 + 6)
        _same(a, ow, ("oracle", t0 + 6), oracle=True)
    # (a tick whose tables did not fit is run again from the collide phase on the candidate lists: it counts in neither)
    assert _numbered(a) == 6 and a.counter("flow6_fallbacks") >= 10, (_numbered(a), a.counter("flow6_fallbacks"))


def test_the_unsplit_launch_keeps_the_scan(ctx):
    """contacts_split = 0: k_contacts_rows reads base, the scan launch stays"""
    from mgf_amd import scenes
    sc = scenes.sphere_pile(5, 5, 8)
    a, b = _run(ctx, sc, 10, {"contacts_split": 0}, 5, 10)
    assert a.counter(NUMBERED) == 0 and a.counter("fused_contacts_ticks") == 10


def test_capsules_keep_the_scan(ctx):
    """k_contacts_rows_index<false>: its slot blocks read base of arbitrary bodies - the scan launch stays (front_rows)"""
    from mgf_amd import scenes
    sc = scenes.capsule_field(8, 6, 8, quads=12, pitch=1.6)
    a, b = _run(ctx, sc, 20, {}, 10, 10)
    assert a.counter("front_rows_ticks") == 20 and a.counter(NUMBERED) == 0 and a.stats.n_constraints > 0
