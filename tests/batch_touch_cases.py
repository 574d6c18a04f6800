"""The definition, the scenes and the sensor layouts of tests/test_gpu_world_batch_touches.py, shared with the CPU check of their conditions
(tests/test_world_batch_touches_host.py): built here so that both see the same inputs.

fold_touch is the contact sensor's report as include/mgf_hip.h defines it ("contact sensors"), restated as a numpy f32 loop with one
operation per statement; layout chooses a world's sensors from that world's own constraint list, deterministically, so that every filter
kind meets sensors with no match, with one and - where the list has them - with several."""
import numpy as np

from mgf_amd._capi import TOUCH_ANY, TOUCH_ANY_BODY, TOUCH_BODY_FRAME, TOUCH_DTYPE, TOUCH_NONE, TOUCH_REPORT_DTYPE, TOUCH_STATIC
from tests.batch_sensor_cases import rotate

f32 = np.float32
PILE_TICKS = (1, 2, 30)
SMALL, MID = 1, 2            # BQ.pile_scenes(): the 96-sphere and the 512-sphere world
NO_SENSOR_WORLD = 0          # ... its world of one body gets no sensor; world 3 has no body and is never named
PARTS_TICK = 60              # a list tick of batch_parts_cases at which the jacks lie on each other
KINDS = ("other", TOUCH_STATIC, TOUCH_ANY_BODY, TOUCH_ANY)


def matches(partner, other):
    if other >= 0:
        return partner == other
    if other == TOUCH_STATIC:
        return partner < 0
    if other == TOUCH_ANY_BODY:
        return partner >= 0
    assert other == TOUCH_ANY
    return True


def chain(cons, x, other):
    """the matching records of body x's chain, in chain order: (list index, x is `a`, partner)"""
    a, b = cons["a"], cons["b"]
    out = [(int(c), True, int(b[c])) for c in np.flatnonzero(a == x)] + [(int(c), False, int(a[c])) for c in np.flatnonzero(b == x)]
    return [r for r in out if matches(r[2], other)]


def fold_touch(cons, q, sensor):
    """mgf_touch_report of `sensor` (a TOUCH_DTYPE record) over its world's constraint list `cons` (CONSTRAINT_DTYPE rows, insertion order)
    and that world's rows q = (s, x, y, z)"""
    x, other, flags = int(sensor["body"]), int(sensor["other"]), int(sensor["flags"])
    out = np.zeros(1, TOUCH_REPORT_DTYPE)
    o = out[0]
    normal = np.ascontiguousarray(cons["normal"], f32)
    nis = np.ascontiguousarray(cons["normal_impulse"], f32)
    imp = np.zeros(3, f32)
    s = f32(0.0)
    n = 0
    best = None
    for c, is_a, partner in chain(cons, x, other):
        ni = nis[c]
        t = normal[c] * ni
        if is_a:
            imp = imp - t
        else:
            imp = imp + t
        s = f32(s + ni)
        if best is None or ni > best[0]:       # (an f32 compare: ties and NaN keep the earlier record)
            best = (ni, c, partner, is_a)
        n += 1
    assert imp.dtype == f32
    if n == 0:
        o["partner"], o["record"] = TOUCH_NONE, -1
        return o
    ni, c, partner, is_a = best
    push = normal[c].copy()
    if is_a:
        push = (push.view(np.uint32) ^ np.uint32(0x80000000)).view(f32)
    arm = np.ascontiguousarray(cons["ra" if is_a else "rb"][c], f32)
    if flags & TOUCH_BODY_FRAME:
        inv = np.ascontiguousarray(q[x], f32) * f32([1.0, -1.0, -1.0, -1.0])
        imp, push, arm = rotate(inv, imp)[0], rotate(inv, push)[0], rotate(inv, arm)[0]
    o["n_contacts"], o["partner"], o["record"] = n, partner, c
    o["impulse"], o["normal_impulse"], o["push"], o["strongest_impulse"], o["arm"] = imp, s, push, ni, arm
    return o


def fold_rig(rig, lists, qs):
    """every sensor of `rig` over its world's list lists[world] and rows qs[world]"""
    out = np.zeros(len(rig), TOUCH_REPORT_DTYPE)
    for i, s in enumerate(rig):
        out[i] = fold_touch(lists[int(s["world"])], qs[int(s["world"])], s)
    return out


def roles(cons, n):
    """per body the list indices where it is `a` and where it is `b`"""
    own, asb = [[] for _ in range(n)], [[] for _ in range(n)]
    for c, (a, b) in enumerate(zip(cons["a"].tolist(), cons["b"].tolist())):
        own[a].append(c)
        if b >= 0:
            asb[b].append(c)
    return own, asb


def strongest_is_late(cons, x):
    """the strongest record of body x's whole chain is not its first"""
    ch = chain(cons, x, TOUCH_ANY)
    ni = cons["normal_impulse"]
    return len(ch) > 1 and any(ni[c] > ni[ch[0][0]] for c, _, _ in ch[1:])


def layout(cons, n, world, spread=10):
    """The sensors of one world of n bodies, from its own list.  Bodies: the first that is both `a` and `b`, whose strongest record is not
    the first of its chain, that is in no record, that has two records against Static, that has records but none against Static, that has
    records against Static only, that meets one body in two records (a manifold) - where the list has such a body - and `spread` more,
    evenly spaced.  Per body: MGF_TOUCH_ANY, _STATIC, _ANY_BODY, the first partner of its own range, the last body it is `b` of, the first
    body it meets in two records and a body it does not touch; the body frame on every other body (on _STATIC: on the others).  The
    first sensor is given again at the end."""
    if n == 0:
        return np.zeros(0, TOUCH_DTYPE)
    own, asb = roles(cons, n)
    b = cons["b"]

    def first(pred):
        return next((x for x in range(n) if pred(x)), None)

    def manifold(x):
        partners = [int(b[c]) for c in own[x] if b[c] >= 0] + [int(cons["a"][c]) for c in asb[x]]
        return len(partners) != len(set(partners))
    special = [first(lambda x: own[x] and asb[x]), first(lambda x: strongest_is_late(cons, x)), first(lambda x: not own[x] and not asb[x]),
               first(lambda x: sum(1 for c in own[x] if b[c] < 0) >= 2), first(lambda x: (own[x] or asb[x]) and all(b[c] >= 0 for c in own[x])),
               first(lambda x: own[x] and not asb[x] and all(b[c] < 0 for c in own[x])), first(manifold)]
    bodies = []
    for x in [s for s in special if s is not None] + np.linspace(0, n - 1, min(n, spread)).astype(int).tolist():
        if x not in bodies:
            bodies.append(int(x))
    rows = []
    for i, x in enumerate(bodies):
        fr = TOUCH_BODY_FRAME if i % 2 else 0
        rows += [(world, x, TOUCH_ANY, fr), (world, x, TOUCH_STATIC, fr ^ TOUCH_BODY_FRAME), (world, x, TOUCH_ANY_BODY, fr)]
        low = [int(b[c]) for c in own[x] if b[c] >= 0]
        high = [int(cons["a"][c]) for c in asb[x]]
        if low:
            rows.append((world, x, low[0], fr))
        if high:
            rows.append((world, x, high[-1], fr ^ TOUCH_BODY_FRAME))
        twice = [y for y in low + high if (low + high).count(y) > 1]
        if twice:
            rows.append((world, x, twice[0], fr))
        touching = set(low + high + [x])
        stranger = first(lambda y: y not in touching)
        if stranger is not None:
            rows.append((world, x, stranger, 0))
    rows.append(rows[0])
    return np.array(rows, TOUCH_DTYPE)


def rig_of(lists, lengths, skip=(), seed=23):
    """the layouts of every world not in `skip`, in one seeded shuffle: sensors in mixed world order"""
    rig = np.concatenate([layout(lists[k], lengths[k], k) for k in range(len(lengths)) if k not in skip] + [np.zeros(0, TOUCH_DTYPE)])
    return rig[np.random.default_rng(seed).permutation(len(rig))]


def many_on_one_world(cons, n, world, count):
    """`count` sensors on one world, more than a work item holds: its layout over every body, then the same in the other frame, cut to
    `count`"""
    rig = layout(cons, n, world, spread=n)
    other = rig.copy()
    other["flags"] ^= TOUCH_BODY_FRAME
    rig = np.concatenate([rig, other])
    assert len(rig) >= count
    return rig[:count].copy()


def hub_sensors(cons, hub, n):
    """on the hub: every record, every body, Static (nothing); between the hub and small spheres from both sides"""
    small = [x for x in (0, 1, 7, 150, 299, 300) if x != hub and x < n]
    rows = [(0, hub, TOUCH_ANY, 0), (0, hub, TOUCH_ANY_BODY, TOUCH_BODY_FRAME), (0, hub, TOUCH_STATIC, 0)]
    for x in small:
        rows += [(0, hub, x, 0), (0, x, hub, TOUCH_BODY_FRAME), (0, x, TOUCH_ANY, 0)]
    rows.append((0, small[0], small[1], 0))          # two small spheres: they do not touch
    return np.array(rows, TOUCH_DTYPE)


def summary(rig, lists):
    """per filter kind the numbers of matches of the rig's sensors of that kind"""
    out = {k: [] for k in KINDS}
    for s in rig:
        other = int(s["other"])
        out["other" if other >= 0 else other].append(len(chain(lists[int(s["world"])], int(s["body"]), other)))
    return out

