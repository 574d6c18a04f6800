"""The contact corpus (tests/contact_corpus.py) proves its own reach on the CPU: the oracle, instrumented with gcov, runs the corpus in a child
process and every executable line of the contact functions has to have run - pair form and world form measured separately, because planting
a case in a world changes it.  Run it alone with

    pytest -m "not gpu" tests/test_contact_corpus.py

The GPU side (tests/test_gpu_contact_corpus.py) then holds every front end of the tick to the oracle on these very inputs."""
import os
import re

import numpy as np
import pytest

from tests import contact_corpus as CC
from tests import oracle_coverage

pytestmark = pytest.mark.skipif(not oracle_coverage.available(), reason="gcov (or g++) is not on this machine: the coverage of the corpus cannot be measured")

ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")

# The contact functions of mgf_collision.hpp: contains(Triangle), ray_sphere, ray_capsule | Plane-Moving<Sphere/Capsule>, last_contact,
# poly_contacts_sphere, seg_2d_intersect, poly_contacts_capsule, the sphere and capsule receivers, the Moving wrappers.
CONTACT_LINES = [(35, 42), (51, 112), (155, 673)]

# ---- lines the pair-level corpus need not reach: one reason per entry -----------------------------------------------------------------
NO_ENTRY = "belongs to a function or instantiation that no entry of the six types reaches"
ALLOWED = {"mgf_collision.hpp": {}, "mgf_math.hpp": {}}
for _l in (177, 178, 179, 180, 182, 183, 185, 186, 187, 189, 190, 191, 192, 193, 196, 197):
    # contacts(Plane, Moving<Capsule>): instantiated only for mgfo_contacts' Plane receiver (pinned by tests/test_oracle_golden.py's vectors);
    # poly_contacts_capsule goes to the plane through the end SPHERES (:293-294), never through this function
    ALLOWED["mgf_collision.hpp"][_l] = NO_ENTRY
ALLOWED["mgf_collision.hpp"][250] = NO_ENTRY   # the Rectangle wrapper of poly_contacts_sphere
ALLOWED["mgf_collision.hpp"][487] = NO_ENTRY   # the Rectangle wrapper of poly_contacts_capsule
for _l in (671, 672):
    # moving_contacts_poly, the commuted form (a moving body as receiver, the polygon as argument): the tick and the corpus put the triangle first
    ALLOWED["mgf_collision.hpp"][_l] = NO_ENTRY
# quat_from_arc's second choice of axis for a half turn.  No input reaches it from the contact functions: their only call is
# quat_from_arc(p.n, (0, 0, 1)) (:337) with |p.n| = 1 (or NaN, which fails every ulps_eq); the half-turn branch needs p.n . z within 4 ulps of
# -|p.n|, i.e. p.n = (~0, ~0, -1), and then cross((1, 0, 0), p.n) = (0, 1, 0) up to rounding - its y is not "ulps_eq 0", so line 138 is skipped.
ALLOWED["mgf_math.hpp"][138] = "unreachable from the contact functions: a unit normal that is -z has cross(x, n) = +y, not zero (see the comment)"

# ---- lines the pair form reaches and the world form need not: why planting loses each ---------------------------------------------------
WORLD_LOSES = {
    # is_zero(ab) after the travel to first touch (:634-636) takes radii that sum to zero (the family cc_zero_radii); a world refuses a body
    # of zero radius (its inertia tensor is singular: physics.rs:212)
    635: "only zero radii reach it, and a world refuses such bodies",
    636: "only zero radii reach it, and a world refuses such bodies",
}
WORLD_MUST_KEEP = [(343, 381), (397, 419), (590, 641)]


def _in(ranges, line):
    return any(lo <= line <= hi for lo, hi in ranges)


@pytest.fixture(scope="module")
def cov():
    with oracle_coverage.Coverage() as c:
        yield c


def _measure(cov, code):
    cov.reset()
    cov.run(code)
    return cov.lines(), cov.functions()


def _missing(lines, funcs):
    """the executable lines of the contact functions, and of every helper of mgf_geom.hpp / mgf_math.hpp they entered, that did not run"""
    out = {"mgf_collision.hpp": sorted(l for l, c in lines["mgf_collision.hpp"].items() if c == 0 and _in(CONTACT_LINES, l))}
    for f in ("mgf_geom.hpp", "mgf_math.hpp"):
        miss = set()
        for start, end, count in funcs[f]:
            if count > 0:
                miss |= {l for l in range(start, end + 1) if lines[f].get(l, 1) == 0}
        out[f] = sorted(miss)
    return out


@pytest.fixture(scope="module")
def pair_form(cov):
    return _measure(cov, "from tests import contact_corpus as C; C.oracle_answers(C.corpus())")


def test_allowlists_hold_only_what_they_may():
    assert set(ALLOWED["mgf_collision.hpp"].values()) == {NO_ENTRY}
    with open(os.path.join(ORACLE, "mgf_collision.hpp")) as f:
        src = f.read().split("\n")
    for line in WORLD_LOSES:
        assert not re.search(r"\bcb\d?\(", src[line - 1]), f"line {line} emits a contact"
        assert not _in(WORLD_MUST_KEEP, line) or line in (635, 636), f"line {line} is one the front ends have to be held to"


def test_pair_form_reaches_every_line_of_the_contact_functions(pair_form):
    lines, funcs = pair_form
    assert any(c > 0 for c in lines["mgf_geom.hpp"].values()) and any(c > 0 for c in lines["mgf_math.hpp"].values())
    missing = _missing(lines, funcs)
    for f, miss in missing.items():
        allowed = ALLOWED.get(f, {})
        unexpected = [l for l in miss if l not in allowed]
        assert not unexpected, f"{f}: the corpus never runs lines {unexpected}"
        stale = [l for l in allowed if l not in miss and lines[f].get(l, 0) > 0]
        assert not stale, f"{f}: lines {stale} are allowed to be missed but ran - drop them from the list"


def test_world_form_reaches_what_the_pair_form_reaches(cov, pair_form):
    pair_lines = {l for l, c in pair_form[0]["mgf_collision.hpp"].items() if c > 0 and _in(CONTACT_LINES, l)}
    lines, _ = _measure(cov, "from tests import contact_corpus as C; C.run_oracle_worlds()")
    world_lines = {l for l, c in lines["mgf_collision.hpp"].items() if c > 0}
    lost = sorted(pair_lines - world_lines)
    unexpected = [l for l in lost if l not in WORLD_LOSES]
    assert not unexpected, f"planted in worlds, the corpus no longer runs lines {unexpected}"


# the worlds of multi-part bodies, each on its own: the union above would hide a scene whose mesh side reaches nothing
TERRAIN_LINES, PAIR_LINES = [(155, 487)], [(493, 642)]
ROUNDING_ONLY = {576: "the second sweep segment parallel by rounding alone (the family of one 1e5-long capsule, which no lattice can hold)"}


@pytest.mark.parametrize("name", ["two_parts", "two_parts_face_grid", "four_parts", "four_parts_face_grid", "seven_parts", "thirty_two_parts",
                                  "three_parts_obstacle"])
def test_each_world_of_multi_part_bodies_reaches_the_branches_on_its_own(cov, pair_form, name):
    """the mesh side of every such world (the obstacle world: its pair side, static receivers) reaches every line the pair form reaches - the
    silhouette clipping :343-381 and the parallel-edge fallback :397-419 among them - and has terrain constraints at every rung"""
    cov.reset()
    cov.run(f"from tests import contact_corpus as C; r = C.run_oracle_worlds(names=['{name}']); assert all(t > 0 for _, t in r.values()), r")
    ran = {l for l, c in cov.lines()["mgf_collision.hpp"].items() if c > 0}
    want = TERRAIN_LINES if name != "three_parts_obstacle" else PAIR_LINES
    pair_lines = {l for l, c in pair_form[0]["mgf_collision.hpp"].items() if c > 0 and _in(want, l)}
    lost = sorted(l for l in pair_lines - ran if l not in WORLD_LOSES and l not in ROUNDING_ONLY)
    assert not lost, f"{name}: planted in this world, the corpus no longer runs lines {lost}"


def test_every_class_of_answer_is_there_for_every_type():
    cases = CC.corpus()
    contacts, counts = CC.oracle_answers(cases)
    assert counts.min() >= 0 and counts.max() <= 2
    cl = CC.classes(cases, contacts, counts)
    for t in CC.TYPES:
        for k in ("none", "t0", "moving"):
            assert cl[t][k] >= 20, (t, k, cl[t])
    assert cl["triangle-capsule"]["two"] >= 20, cl["triangle-capsule"]
    # ... and at every rung of the ladder
    for rung in range(len(CC.LADDER)):
        m = cases["rung"] == rung
        clr = CC.classes(cases[m], contacts[m], counts[m])
        for t in CC.TYPES:
            for k in ("none", "t0", "moving"):
                assert clr[t][k] >= 20, (rung, CC.LADDER[rung], t, k, clr[t])
        assert clr["triangle-capsule"]["two"] >= 20, (rung, clr["triangle-capsule"])


def test_the_corpus_is_deterministic_and_within_its_stated_bounds():
    a, b = CC.corpus(), CC.corpus()
    assert a.tobytes() == b.tobytes()
    fam = np.array(CC.FAMILIES)[a["family"]]
    for f in ("a", "b"):
        v = a[f]["v"]
        assert np.all(np.isfinite(v)) and np.abs(v).max() < 1.1e5 + 200
        assert np.abs(v[fam != "cc_second_sweep_parallel_by_rounding", 3:6][a[f]["kind"][fam != "cc_second_sweep_parallel_by_rounding"] == CC.CAPSULE]).max() <= 200.0
    for f in ("a", "b"):
        r = np.where(a[f]["kind"] == CC.CAPSULE, a[f]["v"][:, 6], a[f]["v"][:, 3])
        body = a[f]["kind"] != CC.TRIANGLE
        assert np.all(r[body & (fam != "cc_zero_radii")] >= 0.002) and np.all(r[body] <= 24.0)
