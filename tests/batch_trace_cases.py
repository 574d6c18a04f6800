"""Shared by the tests of a rollout's touch trace (mgf_batch_rollout_touches / _rollout_touches_dev; WorldBatch.rollout_touches /
.rollout_touches_dev), without a GPU: contact sensor rigs for the scenes of tests/batch_rollout_cases.py and tests/batch_actuator_cases.py,
built from the ORACLE's constraint lists of the ticks a rollout runs - tests/batch_touch_cases.py's layout of several ticks' lists, so
that every filter kind (a named body, TOUCH_STATIC, TOUCH_ANY_BODY, TOUCH_ANY) and both frames meet matches in the course of the rollout
and not only behind its last tick - with more than 256 sensors on world LATE_A (one world, two work items), in one seeded shuffle of the
worlds.  tests/test_world_batch_trace_host.py holds the late-contact rig to the oracle: nothing matches before first contact, every kind
does later, and a report changes from one tick to the next - a row written from the wrong tick shows."""
import functools

import numpy as np

from mgf_amd._capi import TOUCH_BODY_FRAME, TOUCH_DTYPE, TOUCH_REPORT_DTYPE, TOUCH_SHORT_DTYPE
from tests import batch_actuator_cases as AC
from tests import batch_rollout_cases as RC
from tests import batch_touch_cases as TC
from tests.util import oracle_world

# Ticks of a rollout in these tests: RC.T + 2.  By the oracle the late-contact pair first touches at ticks 3 (LATE_A) and 4 (LATE_B), body
# against body; the floor is met at ticks 5 and 7.  Eight ticks hold a match of every filter kind in BOTH worlds - TOUCH_STATIC in LATE_B
# needs tick 7 - and leave both capacity re-runs (ticks 3 and 4 under cons_per_body = 1) in the middle of the call.
T = RC.T + 2
MANY = 260                           # sensors of LATE_A beyond the layouts': with them the world has more than a work item of 256 holds
SHORT_FIELDS = ("n_contacts", "partner", "normal_impulse", "strongest_impulse")


def oracle_ticks(scs, ticks, settle=0):
    """lists[t][k], qs[t][k]: the oracle's constraint list and rows q of world k behind tick settle + t, t < ticks"""
    ows = [oracle_world(sc) for sc in scs]
    for sc, ow in zip(scs, ows):
        for _ in range(settle):
            ow.step(float(sc["dt"]), sc["iters"])
    lists, qs = [], []
    for _ in range(ticks):
        for sc, ow in zip(scs, ows):
            ow.step(float(sc["dt"]), sc["iters"])
        lists.append([ow.constraints() for ow in ows])
        qs.append([ow.state()["q"] for ow in ows])
    return lists, qs


def rig_over_ticks(lists, lengths, many=None, seed=29):
    """the layouts (TC.layout) of every world over the lists of the first tick at which it has a record, of the tick of its longest
    list and of the last tick, then `many` = (world, count) more on one world from every body of it, in both frames;
    all of it in one seeded shuffle"""
    rows = []
    for k, n in enumerate(lengths):
        counts = [len(lists[t][k]) for t in range(len(lists))]
        first = next((t for t in range(len(lists)) if counts[t]), 0)
        for t in sorted({first, int(np.argmax(counts)), len(lists) - 1}):
            rows.append(TC.layout(lists[t][k], n, k))
    if many is not None:
        k, count = many
        t = int(np.argmax([len(lists[t][k]) for t in range(len(lists))]))
        more = np.concatenate([TC.layout(lists[s][k], lengths[k], k, spread=lengths[k]) for s in sorted({t, len(lists) - 1})])
        flipped = more.copy()
        flipped["flags"] ^= TOUCH_BODY_FRAME
        more = np.concatenate([more, flipped])
        assert len(more) >= count, (len(more), count)
        rows.append(more[:count])
    rig = np.concatenate(rows + [np.zeros(0, TOUCH_DTYPE)])
    return np.ascontiguousarray(rig[np.random.default_rng(seed).permutation(len(rig))])


@functools.lru_cache(maxsize=None)
def _late():
    scs = RC.late_contact_scenes()
    lists, qs = oracle_ticks(scs, T)
    lengths = [len(sc["comps"]) for sc in scs]
    return scs, lists, qs, rig_over_ticks(lists, lengths, many=(RC.LATE_A, MANY))


def late_touch_rig():
    """the rig of RC.late_contact_scenes(): a copy"""
    return _late()[3].copy()


def late_oracle():
    """(scenes, lists[t][k], qs[t][k]) of RC.late_contact_scenes() by the oracle, no actuator acting; not to be written to"""
    return _late()[:3]


@functools.lru_cache(maxsize=None)
def _actuator():
    scs = AC.actuator_scenes()
    lists, qs = oracle_ticks(scs, T, settle=AC.TICKS)
    return rig_over_ticks(lists, [len(sc["comps"]) for sc in scs], seed=31)


def actuator_touch_rig():
    """the rig of AC.actuator_scenes() behind their AC.TICKS ticks (the oracle's worlds without the spin, the bodies added late and
    the actuation of the GPU test: the sensors name bodies that lie on the ground or on each other in both): a copy"""
    return _actuator().copy()


def fold_ticks(rig, lists, qs):
    """[T, n] reports: TC.fold_rig of every tick"""
    out = np.zeros((len(lists), len(rig)), TOUCH_REPORT_DTYPE)
    for t in range(len(lists)):
        out[t] = TC.fold_rig(rig, lists[t], qs[t])
    return out


def short_of(full):
    """the short rows of full ones: the four named words"""
    out = np.zeros(full.shape, TOUCH_SHORT_DTYPE)
    for f in SHORT_FIELDS:
        out[f] = full[f]
    return out


def kind(sensor):
    other = int(sensor["other"])
    return "other" if other >= 0 else other
