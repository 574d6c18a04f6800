"""Wide bodies that meet each other (WideSpec in k_bodies.h, k_pair_wide in k_front_rows.h): two runaways flying at each other, a fast one
catching a slow one, random runaways by the dozen, the list filled to its last record and one past it.  A wide i whose tight box meets
the fat box of a wide j can have its centre far outside fat_j grown by rmax - the reach of k_pair_wide's cell walk - so the scripted
scenes put the pair exactly there (tests/wide_pairs.py) and check it from the oracle's boxes before they judge the world.

Every tick three worlds agree: the HIP world with the list, the same with `wide_list` off, and the oracle - the counts of pair candidates
and constraints, and the bits of x, q, v, omega; around the meeting tick and every few ticks the constraint lists with their impulses."""
import numpy as np
import pytest

from tests import wide_pairs as W
from tests.util import compare_constraints, oracle_world, values_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import mgf_amd
    c = mgf_amd.Context(0)
    yield c
    c.close()


def _same(x, y):
    return all(np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)) for k in ("x", "q", "v", "omega"))


def _three_way(ctx, sc, ticks, options=(), check=lambda tick, ow: None, full_every=3, full_at=()):
    """runs the list-on world, the list-off world and the oracle side by side; `check(tick, ow)` after the oracle's build_constraints
    -> (list-on world, the most wide bodies it listed in one tick)"""
    import mgf_amd
    dt, it = float(sc["dt"]), sc["iters"]
    a, b = mgf_amd.World.from_scene(ctx, sc), mgf_amd.World.from_scene(ctx, sc)
    for k, v in options:
        a.set_option(k, v); b.set_option(k, v)
    b.set_option("wide_list", 0)
    ow = oracle_world(sc)
    peak = 0
    for s in range(ticks):
        so = ow.build_constraints(dt)
        want = (so.n_pair_candidates, so.n_constraints)
        check(s, ow)
        sa, sb = a.build_constraints(dt), b.build_constraints(dt)
        on, off = (sa.n_pair_candidates, sa.n_constraints), (sb.n_pair_candidates, sb.n_constraints)
        assert on == off, f"tick {s}: list on {on}, list off {off}, oracle {want}"
        assert on == want, f"tick {s}: list on and off {on}, oracle {want}"
        ow.solve(it); a.solve(it); b.solve(it)
        if s % full_every == 0 or s in full_at:
            oc = ow.constraints()
            compare_constraints(a.constraints(), b.constraints(), check_impulse=True)
            compare_constraints(a.constraints(), oc, check_impulse=True)
        g, o = a.state(), ow.state()
        assert _same(g, b.state()), f"tick {s}: the list on and off differ"
        for k in ("x", "q", "v", "omega"):
            assert values_equal(g[k], o[k]), f"tick {s}: {k} differs from the oracle"
        peak = max(peak, a.counter("wide_bodies"))
    return a, peak


def _meeting(ctx, kind, motion, fast_larger, options=()):
    sc, (i, j) = W.meeting_scene(kind, motion, fast_larger)
    seen = []

    def check(s, ow):
        if s == W.MEET_TICK:
            seen.append(W.lost_region_checks(ow, i, j, (i, j), W.min_margin(kind)))
    a, peak = _three_way(ctx, sc, W.MEET_TICK + 6, options, check, full_at=range(W.MEET_TICK - 1, W.MEET_TICK + 3))
    assert seen, "the meeting tick was not checked"
    assert a.counter("wide_ticks") > 0 and peak >= 2 and a.counter("wide_overflows") == 0, (a.counter("wide_ticks"), peak, a.counter("wide_overflows"))


@pytest.mark.parametrize("fast_larger", [True, False], ids=["fast_has_larger_id", "fast_has_smaller_id"])
@pytest.mark.parametrize("motion", ["head_on", "catch_up"])
@pytest.mark.parametrize("kind", W.KINDS)
def test_wide_bodies_that_meet_equal_the_oracle(ctx, kind, motion, fast_larger):
    _meeting(ctx, kind, motion, fast_larger)


@pytest.mark.parametrize("motion", ["head_on", "catch_up"])
def test_wide_bodies_that_meet_in_a_resorted_world(ctx, motion):
    """resort_every 3: slots and order ids differ (Lbvh::ext) - k_pair_wide reads the order ids through it"""
    _meeting(ctx, "spheres", motion, False, options=(("resort_every", 3),))


# seeds of tools/wide_pairs_fuzz.py whose runaways stay few enough for the list: where they knock more than kWideCap bodies of the pile
# into flight the list overflows and rests for 64 ticks (by design: no outliers then), and k_pair_wide is not what such a seed tests
FUZZ_SEEDS = [("spheres", s) for s in (0, 6, 8, 12, 14, 24, 28, 30, 38, 40)] + [("two_part_bodies", s) for s in (1, 3, 5, 7, 9)]


@pytest.mark.parametrize("base,seed", FUZZ_SEEDS)
def test_random_runaways_equal_the_oracle(ctx, base, seed):
    sc, _ = W.fuzz_scene(W.FUZZ_SEED_BASE + seed, base)
    a, _ = _three_way(ctx, sc, 32, full_every=4)
    assert a.counter("wide_ticks") > 0, "no tick ran with the list"


def _far_runaways(k):
    """a 12^3 pile with k of its spheres far below, 20 m apart, falling at 200 m/s: each of them wide, none near another"""
    from mgf_amd import scenes
    base = scenes.sphere_pile(12, 12, 12)
    movers = [(3 + 17 * a, (-80.0 + 20.0 * (a % 9), W.FAR_Y, -80.0 + 20.0 * (a // 9)), (0.0, -200.0, 0.0), ("sphere", 0.5)) for a in range(k)]
    return W.place(base, movers)


def test_a_full_list_runs_without_overflow(ctx):
    """exactly kWideCap = 64 wide bodies: listed, no re-run"""
    a, peak = _three_way(ctx, _far_runaways(64), 10)
    assert a.counter("wide_overflows") == 0 and a.counter("wide_ticks") > 0, (a.counter("wide_overflows"), a.counter("wide_ticks"))
    assert peak == 64, peak


def test_one_past_the_list_runs_again_without_it(ctx):
    """65 wide bodies: the tick fails and runs again without the list"""
    a, _ = _three_way(ctx, _far_runaways(65), 10)
    assert a.counter("wide_overflows") >= 1, a.counter("wide_overflows")
