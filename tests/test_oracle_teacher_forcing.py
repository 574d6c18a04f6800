"""The teacher-forcing route of the GPU window tests (test_gpu_bench_windows.py) and of bench.py's CPU sample of config 3, on the
oracle alone: a fresh world handed a stepped world's state with set_state (x, q, v, omega, delta) must step on exactly as the world
that reached that state by stepping - the same constraint lists (impulses included) and the same state bits - although its fat boxes
and BVH come from its own, different history.  The scene is config 3's bench scene (capsules over a heightfield, default y0) at a
size the oracle steps in milliseconds."""
from tests.util import compare_constraints, oracle_world, rel_err, values_equal

FIELDS = ("x", "q", "v", "omega", "delta")


def test_set_state_then_step_equals_stepping_there():
    from mgf_amd import scenes
    scene = scenes.capsule_field(12, 4, 12, quads=16)
    dt, iters = float(scene["dt"]), scene["iters"]
    ref = oracle_world(scene)
    for _ in range(90):  # (the capsules have landed on the heightfield and on each other)
        ref.step(dt, iters)
    forced = oracle_world(scene)
    forced.set_state(**ref.state())
    for t in range(5):
        a, b = ref.step(dt, iters), forced.step(dt, iters)
        ca, cb = (int(a.n_constraints), int(a.n_terrain_constraints)), (int(b.n_constraints), int(b.n_terrain_constraints))
        assert ca == cb, f"tick {t}: stepped (constraints, terrain) {ca}, teacher-forced {cb}"
        assert ca[0] > 300 and ca[1] > 100 and ca[0] > ca[1], ca  # body-body and body-terrain contacts both present
        compare_constraints(forced.constraints(), ref.constraints(), check_impulse=True)
        s, f = ref.state(), forced.state()
        for k in FIELDS:
            assert values_equal(f[k], s[k]), f"tick {t}: {k} differs (rel err {rel_err(f[k], s[k]):.3g})"
