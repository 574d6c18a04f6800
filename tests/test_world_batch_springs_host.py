"""The springs of a batch (mgf_batch_set_springs, mgf_batch_spring_count, mgf_batch_apply_springs, mgf_batch_apply_springs_dev) without
a GPU: the header, the library, the binding and the documents carry the calls and the record of 64 bytes; the numpy restatement of the
wrench (tests/batch_spring_cases.py) gives the fixed cases of the definition; the plan of the ends is runs of one body in list order;
what needs no device is refused, in the header's order, with the rig unchanged; and the kernels have the actuators' loop shape."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_spring_cases as SP
from tests.util import ROOT, kernel_resources, read

f32 = np.float32
CALLS = ("mgf_batch_set_springs", "mgf_batch_spring_count", "mgf_batch_apply_springs", "mgf_batch_apply_springs_dev")
RIG_FILE = "host_batch_spring.inc"
IDENT = f32([1, 0, 0, 0])


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls_and_the_record():
    h = read("include", "mgf_hip.h")
    flat_h = re.sub(r"\s+", " ", h)
    for sig in ("MGF_API mgf_status mgf_batch_set_springs(mgf_batch* b, const mgf_batch_spring* s, int64_t n);",
                "MGF_API int64_t mgf_batch_spring_count(const mgf_batch* b);",
                "MGF_API mgf_status mgf_batch_apply_springs(mgf_batch* b, float h, float* wrench_out);",
                "MGF_API mgf_status mgf_batch_apply_springs_dev(mgf_batch* b, float h, float* wrench_out_dev);"):
        assert sig in flat_h, sig
    # a section of its own, behind the rollouts' declarations and ahead of the counters
    assert h.index("MGF_API mgf_status mgf_batch_rollout_dev(") < h.index("/* ---- springs between bodies") < h.index("/* name in {")
    for name, value in (("MGF_BATCH_SPRING_LAUNCHES", _capi.BATCH_SPRING_LAUNCHES), ("MGF_BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK", _capi.BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK),
                        ("MGF_BATCH_ROLLOUT_LAUNCHES_PER_TICK", _capi.BATCH_ROLLOUT_LAUNCHES_PER_TICK)):
        m = re.search(r"#define %s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == value == 2, name
    assert "with an empty spring rig" in h[h.index("#define MGF_BATCH_ROLLOUT_LAUNCHES_PER_TICK"):h.index("MGF_API mgf_status mgf_batch_rollout(")]
    section = h[h.index("/* ---- springs between bodies"):h.index("/* name in {")]
    for word in ("ra = rotate(q_a, pa);  Pa = x_a + ra;  Va = v_a + cross(omega_a, ra)", "Pb = pb;  Vb = (0,0,0)", "len = sqrt(dot(d, d));  n = d / len",
                 "rate = dot(Vb - Va, n)", "f = k * (len - rest) + c * rate;  if (f < lo) f = lo;  if (f > hi) f = hi", "a NaN stays a NaN", "s = f * h",
                 "L = n * s;  A = cross(ra, L)", "Lb = -L;  Ab = cross(rb, Lb)", "springs_skipped", "bit for bit", "mgf_batch_apply_impulses",
                 "untouched to the bit", "several components", "drive_launches", "rollout_launches", "the rig was not changed", "nothing enqueued",
                 "mgf_batch_add_bodies", "no float atomic", "Rotation::rotate_vector", "mgf_batch_apply_springs_dev(b, dt, NULL)", "ONCE",
                 "mgf_batch_step itself stays World::step, launch for launch", "OUT OF SCOPE", "hard joints", "lone mgf_world", "inside mgf_batch_step",
                 "torsion", "driven per tick"):
        assert word in section, word
    assert '"springs_skipped"' in h[h.index("/* name in {"):]
    # the record: 64 bytes, the same fields at the same offsets in the ctypes struct and the numpy dtype
    assert C.sizeof(_capi.BatchSpring) == 64 == _capi.SPRING_DTYPE.itemsize
    names = ["world", "body", "other", "flags", "pa", "rest", "pb", "k", "c", "lo", "hi", "pad"]
    assert [f[0] for f in _capi.BatchSpring._fields_] == list(_capi.SPRING_DTYPE.names) == names
    want_off = [0, 4, 8, 12, 16, 28, 32, 44, 48, 52, 56, 60]
    assert [_capi.SPRING_DTYPE.fields[k][1] for k in names] == want_off == [getattr(_capi.BatchSpring, k).offset for k in names]
    assert re.search(r"typedef struct mgf_batch_spring \{\s*int32_t world, body, other; uint32_t flags;[^\n]*\n\s*mgf_vec3 pa; float rest;[^\n]*\n\s*mgf_vec3 pb; float k;[^\n]*\n"
                     r"\s*float c, lo, hi, pad;[^\n]*\n\} mgf_batch_spring;", h)
    lib = mgf_amd.load_library()
    vp, i64, i32, fl = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    want = {"mgf_batch_set_springs": (i32, [vp, vp, i64]), "mgf_batch_spring_count": (i64, [vp]),
            "mgf_batch_apply_springs": (i32, [vp, fl, vp]), "mgf_batch_apply_springs_dev": (i32, [vp, fl, vp])}
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == want[name], name
    for method in ("set_springs", "spring_count", "apply_springs", "apply_springs_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    for name in ("SPRING_DTYPE", "BATCH_SPRING_LAUNCHES", "BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK"):
        assert getattr(mgf_amd, name) is getattr(_capi, name), name
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for sig in ("pub fn mgf_batch_set_springs(b: *mut mgf_batch, s: *const mgf_batch_spring, n: i64) -> mgf_status;",
                "pub fn mgf_batch_spring_count(b: *const mgf_batch) -> i64;",
                "pub fn mgf_batch_apply_springs(b: *mut mgf_batch, h: f32, wrench_out: *mut f32) -> mgf_status;",
                "pub fn mgf_batch_apply_springs_dev(b: *mut mgf_batch, h: f32, wrench_out_dev: *mut f32) -> mgf_status;",
                "pub struct mgf_batch_spring { pub world: i32, pub body: i32, pub other: i32, pub flags: u32, pub pa: mgf_vec3, pub rest: f32, pub pb: mgf_vec3, "
                "pub k: f32, pub c: f32, pub lo: f32, pub hi: f32, pub pad: f32 }",
                "pub const MGF_BATCH_SPRING_LAUNCHES: i64 = 2;", "pub const MGF_BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK: i64 = 2;",
                "pub fn set_springs(", "pub fn spring_count(", "pub fn apply_springs(", "pub unsafe fn apply_springs_dev("):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_rollout.h"') < kernels.index('#include "k_batch_spring.h"')
    assert "k_batch_spring_wrench / k_batch_spring_apply<GATED> (k_batch_spring.h)" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_rollout.inc"') < hip.index('#include "%s"' % RIG_FILE)
    design = read("DESIGN.md")
    assert design.index("## Rollouts") < design.index("## Springs") < design.index("## 9.")
    sub = design[design.index("## Springs"):design.index("## 9.")]
    for word in ("k_batch_spring_wrench", "k_batch_spring_apply", "done[k] == t && act[k] == t", "Compiler output", "Out of scope", "batch_spring_bench.py",
                 "MGF_BATCH_SPRING_LAUNCHES", "MGF_BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK", "__any", "bench.py"):
        assert word in sub, word
    readme = read("README.md")
    assert "set_springs" in readme and "apply_springs_dev" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_spring_bench.py"))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def _pair(xa, xb, qa=IDENT, qb=IDENT, va=(0, 0, 0), vb=(0, 0, 0), oa=(0, 0, 0), ob=(0, 0, 0)):
    return f32([xa, xb]), f32([qa, qb]), f32([va, vb]), f32([oa, ob])


def test_the_restatement_gives_the_fixed_cases_of_the_definition():
    h = f32(1.0 / 60.0)
    # a spring at rest with no relative velocity: zeros, and not a skip
    st = _pair((0, 0, 0), (0, 2, 0), va=(1, 2, 3), vb=(1, 2, 3))
    W, sk = SP.wrenches(SP.spring(0, 0, 1, rest=2.0, k=50.0, c=20.0), h, *st, [2])
    assert not W.any() and not sk.any()
    # stretched, turned and moving: Lb == -L to the bit, the pull on `body` points at the far end, both torques are cross(arm, impulse)
    q = f32([0.5, 0.5, -0.5, 0.5])
    st = _pair((0.1, 0.2, 0.3), (1.7, -0.4, 2.2), qa=q, qb=q[[0, 3, 1, 2]], va=(0.3, -1, 2), vb=(-2, 0.5, 0.1), oa=(3, -4, 5), ob=(-1, 2, 7))
    r = SP.spring(0, 0, 1, pa=(0.3, -0.2, 0.1), pb=(-0.1, 0.25, 0.3), rest=0.7, k=31.0, c=2.5)
    W, sk = SP.wrenches(r, h, *st, [2])
    assert not sk.any() and np.all(W != 0) and W.dtype == f32
    assert W[0, 6:9].tobytes() == (-W[0, 0:3]).tobytes()
    ra, rb = SP.SC.rotate(st[1][0:1], r["pa"]), SP.SC.rotate(st[1][1:2], r["pb"])
    d = (st[0][1] + rb[0]) - (st[0][0] + ra[0])
    assert np.dot(W[0, 0:3].astype(np.float64), d.astype(np.float64)) > 0              # f > 0 here: pulled towards the far end
    assert W[0, 3:6].tobytes() == SP.SC._cross(ra, W[:, 0:3])[0].tobytes() and W[0, 9:12].tobytes() == SP.SC._cross(rb, W[:, 6:9])[0].tobytes()
    # against float64: the f32 sequence is the formula
    x64, v64, o64 = (a.astype(np.float64) for a in (st[0], st[2], st[3]))
    ra64, rb64 = ra[0].astype(np.float64), rb[0].astype(np.float64)
    d64 = (x64[1] + rb64) - (x64[0] + ra64)
    ln = np.linalg.norm(d64)
    rate = np.dot((v64[1] + np.cross(o64[1], rb64)) - (v64[0] + np.cross(o64[0], ra64)), d64 / ln)
    L64 = d64 / ln * (31.0 * (ln - 0.7) + 2.5 * rate) * (1.0 / 60.0)
    assert np.allclose(W[0, 0:3], L64, rtol=1e-4, atol=1e-6)
    # a world anchor has no far record and zeros for its far end
    a = SP.spring(0, 1, -1, pa=(0.1, 0, 0), pb=(5, 5, 5), rest=1.0, k=10.0)
    W, sk = SP.wrenches(a, h, *st, [2])
    assert W[0, 0:3].all() and W[0, 3:6].any() and not W[0, 6:12].any() and not sk.any()
    w, b, lin, ang = SP.records(np.concatenate([r, a, r]), np.concatenate([W, W, W]))
    assert w.tolist() == [0] * 5 and b.tolist() == [0, 1, 1, 0, 1] and lin.shape == ang.shape == (5, 3)
    # len == 0 is skipped: an anchor at the body's own point
    z = SP.spring(0, 0, -1, pb=st[0][0], rest=0.0, k=10.0)
    W, sk = SP.wrenches(z, h, *st, [2])
    assert sk.tolist() == [True] and not W.any()
    # the clamps: a rope does not push, a strut does not pull, a finite clamp saturates; -inf / inf clamp nothing
    st = _pair((0, 0, 0), (0.5, 0, 0))
    free, _ = SP.wrenches(SP.spring(0, 0, 1, rest=1.0, k=40.0), h, *st, [2])
    rope, sk = SP.wrenches(SP.spring(0, 0, 1, rest=1.0, k=40.0, lo=0.0), h, *st, [2])
    assert free[0, 0] < 0 and not rope.any() and not sk.any()                           # compressed: the free spring pushes `body` away
    st = _pair((0, 0, 0), (3, 0, 0))
    strut, sk = SP.wrenches(SP.spring(0, 0, 1, rest=1.0, k=40.0, hi=0.0), h, *st, [2])
    sat, _ = SP.wrenches(SP.spring(0, 0, 1, rest=1.0, k=40.0, lo=-1.5, hi=1.5), h, *st, [2])
    assert not strut.any() and not sk.any() and sat[0, 0].tobytes() == (f32(1.5) * h).tobytes()
    # a NaN gain product gives a zero wrench and a skip: k * len = +inf beside c * rate = -inf; so does an overflow alone
    st = _pair((0, 0, 0), (10, 0, 0), va=(-20, 0, 0))
    for r in (SP.spring(0, 0, 1, k=3.0e38, c=-3.0e38), SP.spring(0, 0, 1, k=3.0e38), SP.spring(0, 0, -1, pb=(10, 0, 0), k=3.0e38, c=-3.0e38)):
        W, sk = SP.wrenches(r, h, *st, [2])
        assert sk.tolist() == [True] and not W.any() and np.all(np.isfinite(W))
    # ... while a clamp brings an infinite force back: not a skip
    W, sk = SP.wrenches(SP.spring(0, 0, 1, k=3.0e38, hi=2.0), h, *st, [2])
    assert not sk.any() and W[0, 0].tobytes() == (f32(2.0) * h).tobytes()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_plan_of_the_ends_is_runs_of_one_body_in_list_order():
    lens = list(SP.LENGTHS)
    total = sum(lens)
    x = np.random.default_rng(1).uniform(-3, 3, (total, 3)).astype(f32)
    _, v, _ = SP.written_state(total)
    rig, planted = SP.main_rig(lens, x, v)
    n = len(rig)
    assert 190 <= n <= 230 and len(set(planted)) == 3 and np.all(rig["other"][planted] == -1)
    assert set(rig["world"].tolist()) == {0, 1, 2, 3} and np.any(np.diff(rig["world"]) < 0)
    assert np.all(rig["body"] < np.int64(lens)[rig["world"]]) and np.all(rig["other"] < np.int64(lens)[rig["world"]]) and np.all(rig["other"] != rig["body"])
    assert 10 <= int(np.sum(rig["other"] < 0)) <= 40 and np.any(rig["lo"] == 0) and np.any(rig["hi"] == 0) and np.any(np.isinf(rig["lo"]) & np.isinf(rig["hi"]))
    runs, order = SP.end_plan(rig)
    n_ends = 2 * n - int(np.sum(rig["other"] < 0))
    assert sorted(order.tolist()) == sorted(2 * i + s for i in range(n) for s in (0, 1) if s == 0 or rig["other"][i] >= 0) and len(order) == n_ends
    seen = np.zeros(n_ends, np.int64)
    for w, b, first, count in runs:
        e = order[first:first + count]
        assert count >= 1 and np.all(np.diff(e) > 0)                                 # list order within a run: ascending end index
        assert np.all(rig["world"][e >> 1] == w) and np.all(np.where(e & 1, rig["other"][e >> 1], rig["body"][e >> 1]) == b)
        seen[first:first + count] += 1
    assert np.all(seen == 1)
    keys = runs[:, 0] * 4096 + runs[:, 1]
    assert np.all(np.diff(keys) > 0)                                                 # one run a body, sorted by (world, body)
    assert len(runs) == sum(lens[:4]) > 64                                           # every body of the four worlds: more than a wave of runs
    hub = runs[(runs[:, 0] == SP.HUB[0]) & (runs[:, 1] == SP.HUB[1])][0]
    assert hub[3] >= SP.HUB_ENDS > 64                                                # a run longer than a wave
    sides = order[hub[2]:hub[2] + hub[3]] & 1
    assert sides.min() == 0 and sides.max() == 1                                     # the hub is `body` of some and `other` of others
    # springs whose two ends belong to lanes of different waves
    run_of = {(int(r[0]), int(r[1])): k for k, r in enumerate(runs)}
    far = np.flatnonzero(rig["other"] >= 0)
    split = [i for i in far if run_of[(int(rig["world"][i]), int(rig["body"][i]))] // 64 != run_of[(int(rig["world"][i]), int(rig["other"][i]))] // 64]
    assert len(split) >= 1
    # the planted springs are skipped by the restatement whatever q and omega are; nothing else is
    q, v, om = SP.written_state(total)
    W, sk = SP.wrenches(rig, 1.0 / 60.0, x, q, v, om, lens)
    assert sorted(np.flatnonzero(sk).tolist()) == sorted(planted) and np.all(np.isfinite(W)) and not W[planted].any()
    free = ~sk & np.isinf(rig["lo"]) & np.isinf(rig["hi"])
    assert np.all(np.any(W[free][:, 0:3] != 0, axis=1)) and np.any(W[~free & ~sk] != 0) and np.any(~W[~free & ~sk].any(axis=1))   # some clamps bite, some do not
    # the host's plan is that plan: a stable sort by (world, body) of the ends, reached behind every check
    src = read("mgf_amd", "csrc", RIG_FILE)
    plan = src[src.index("static void batch_spring_plan("):src.index('extern "C" mgf_status mgf_batch_set_springs(')]
    assert "std::stable_sort(" in plan and plan.index("std::stable_sort(") < plan.index("R.recs.assign(") < plan.index("R.stale = true;")
    assert "if (recs[i].other >= 0) order.push_back((uint32_t)(2 * i + 1));" in plan
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(", plan)
    # the scenes: five worlds of 8 to 24 bodies, spheres and capsules, and a world without bodies
    scs = SP.spring_scenes()
    assert [len(sc["comps"]) for sc in scs] == lens and lens[SP.EMPTY_WORLD] == 0 and all(8 <= c <= 24 for c in lens[:5])
    assert all(set(sc["comps"]["tag"].tolist()) == {0, 1} for sc in scs[:5])
    for count in (1, 256, 257, 600):
        r = SP.sized_rig(lens, count)
        assert len(r) == count and np.all(r["other"] != r["body"]) and np.all(r["other"] < np.int64(lens)[r["world"]]) and np.all(r["body"] < np.int64(lens)[r["world"]])
    lr, lp = SP.late_springs([27, 18, 8])
    assert len(lr) == 45 and set(lr["world"].tolist()) == {0, 1, 2} and np.all(lr["other"] != lr["body"]) and np.all(lr["k"][[i for i in range(45) if i not in lp]] <= 0.3)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_device_is_refused_in_the_headers_order_with_the_rig_unchanged():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced
    rig = np.zeros(4, _capi.SPRING_DTYPE)
    out = C.c_void_p(1 << 21)
    h = C.c_float(1.0 / 60.0)
    assert lib.mgf_batch_spring_count(None) == -1
    assert lib.mgf_batch_set_springs(None, rig.ctypes.data, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_springs(None, None, 0) == INV and "NULL" in err()
    assert lib.mgf_batch_set_springs(fake, None, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_springs(fake, rig.ctypes.data, -1) == INV and "negative" in err()
    assert lib.mgf_batch_set_springs(fake, rig.ctypes.data, 1 << 31) == INV and "too many" in err()
    for fn in (lib.mgf_batch_apply_springs, lib.mgf_batch_apply_springs_dev):
        assert fn(None, h, out) == INV and "NULL" in err()
        assert fn(None, C.c_float(np.nan), None) == INV and "NULL" in err()                  # the handle first
        for bad in (np.nan, np.inf, -np.inf):
            assert fn(fake, C.c_float(bad), out) == INV and "h is not finite" in err(), bad
    # what needs the handle's contents is refused on the host too, every record ahead of any change of the rig and of any device work
    # (read here; run in tests/test_gpu_world_batch_springs.py, where a handle exists)
    src = read("mgf_amd", "csrc", RIG_FILE)
    body = src[src.index('extern "C" mgf_status mgf_batch_set_springs('):src.index('extern "C" int64_t mgf_batch_spring_count(')]
    plan_call = "batch_spring_plan(b->springs, sp, n);"
    assert not re.search(r"b->springs\.|\bR\.", body.replace(plan_call, ""))                 # the rig changes in the plan step alone
    marks = ["batch_rig_set_args(b, sp, n_in)", 'batch_rig_ref_check(b, r.world, r.body, 0, "spring")', "r.other < -1 || (r.other >= 0 && (uint32_t)r.other >= b->h_n[(size_t)r.world])",
             "r.other == r.body", "r.flags != 0u", "a spring's pa, pb, k, c or rest is not finite: the rig was not changed", "r.rest < 0.0f",
             "a spring's lo or hi is a NaN, or lo > hi: the rig was not changed", plan_call]
    order = [body.index(s) for s in marks]
    assert order == sorted(order), order
    assert body.count("the rig was not changed") == 6
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(", body)                      # no device work at all
    # what tests/test_world_batch_rigs_host.py asks of a rig file: the shared steps used, not copied
    assert src.count("batch_rig_set_args(b, ") == 1 and src.count("batch_rig_up(b, R, ") == 1 and 'batch_rig_up(b, R, "spring", 3)' in src
    for gone in ("BatchQueryPlan plan(", "batch_rig_upload(", "names a body its world does not hold", '"batch is NULL"'):
        assert gone not in src, gone
    for fn in ("batch_rig_set_args", "batch_rig_ref_check", "batch_rig_plan", "batch_rig_upload", "batch_rig_up", "batch_rig_handle", "batch_rig_cap", "batch_rig_fits"):
        assert not re.search(r"^static \w+ " + fn + r"\(", src, re.M), fn
    # the far ends are held against the lengths again when the rig goes up behind added bodies
    ready = src[src.index("static mgf_status batch_spring_ready("):src.index("static mgf_status batch_spring_run(")]
    assert ready.index("(uint32_t)R.recs[i].other >= b->h_n[(size_t)R.recs[i].world]") < ready.index("batch_rig_up(")
    host = read("mgf_amd", "csrc", "host_batch.inc")
    stale = host[host.index("static void batch_rigs_stale("):host.index('extern "C" mgf_status mgf_batch_add_bodies(')]
    assert host.count("BatchRig<mgf_batch_spring> springs;") == 1 and "b->springs.stale = true;" in stale
    assert '"springs_skipped"' in host[host.index('extern "C" mgf_status mgf_batch_counter('):]
    # the apply calls: the refusals, the context, (device form) the pointer looked up - and only then the first thing is enqueued
    enqueue = r"batch_spring_run\(|batch_spring_ready\(|batch_rig_up\(|batch_push\(|hipMemsetAsync|hipMemcpyAsync|<<<|\.ensure\(|h2d\("
    dev = src[src.index('extern "C" mgf_status mgf_batch_apply_springs_dev('):]
    first_enqueue = min(m.start() for m in re.finditer(enqueue, dev))
    assert dev.index("batch_spring_args(b, h)") < dev.index("ctx_bind(") < dev.index('dev_span(b->ctx, wrench_out_dev, 48 * n, "wrench_out_dev")') < first_enqueue
    assert dev.index("if (n == 0) return MGF_OK;") < first_enqueue and "hipStreamSynchronize" not in dev and "hipMemcpy" not in dev
    host_form = src[src.index('extern "C" mgf_status mgf_batch_apply_springs('):src.index('extern "C" mgf_status mgf_batch_apply_springs_dev(')]
    assert host_form.count("hipStreamSynchronize") == 1 and host_form.count("hipMemcpyDeviceToHost") == 1 and "hipMemcpyHostToDevice" not in host_form
    assert host_form.index("if (n == 0) return MGF_OK;") < host_form.index("batch_spring_run(")
    run = src[src.index("static mgf_status batch_spring_run("):src.index("static mgf_status batch_spring_args(")]
    assert run.count("<<<") == 2 and run.index("batch_push(") < run.index("batch_spring_ready(") < run.index("k_batch_spring_wrench<<<") < run.index("k_batch_spring_apply<false><<<")
    assert "b->d_launches += MGF_BATCH_SPRING_LAUNCHES;" in run and "batch_single_parts(" not in src
    # the rollout: the springs' launches ride in the step's train ahead of the actuation, through the hook
    roll = read("mgf_amd", "csrc", "host_batch_rollout.inc")
    core = roll[roll.index("static mgf_status batch_rollout_run("):roll.index('extern "C" mgf_status mgf_batch_rollout_dev(')]
    assert "!b->springs.recs.empty()" in core and core.index("batch_push(") < core.index("batch_spring_ready(b, dt, nullptr, &H.S)") < core.index("batch_step_run(b, dt, iters, n_ticks, stats, &H)")
    train = host[host.index("static mgf_status batch_step_run("):host.index('extern "C" mgf_status mgf_batch_step(')]
    assert train.index("k_batch_spring_wrench<<<") < train.index("k_batch_spring_apply<true><<<") < train.index("k_batch_rollout_act<") < train.index("batch_collide(")
    assert "hook->launches += MGF_BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK;" in train and train.count("k_batch_spring_") == 2


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_kernels_have_the_actuators_loop_shape_and_no_float_atomic():
    k = read("mgf_amd", "csrc", "k_batch_spring.h")
    body = k[k.index("void k_batch_spring_apply("):]
    body = body[:body.index("\n}\n")]
    assert body.count("return;") == 1 and body.index("__any(j < cnt)") < body.index("if (j < cnt)") < body.index("if (!live) return;")
    assert "__syncthreads" not in body and "break" not in body and "continue" not in body and "atomic" not in body
    assert "A.done[run.x] == A.tick && A.act[run.x] == A.tick" in body and "const uint32_t cnt = live ? run.w : 0u;" in body
    assert "lin + L * inv_mass" in body and "ang + I * T" in body and not re.search(r"A\.act\[[^\]]+\] =[^=]", k)
    loop = body[body.index("__any(j < cnt)"):body.index("if (!live) return;")]
    assert "GATED" not in loop and "A.done" not in loop                               # nothing wave-uniform is evaluated inside the loop
    wrench = k[k.index("void k_batch_spring_wrench("):k.index("template <bool GATED>")]
    assert re.findall(r"atomic\w*\(", wrench) == ["atomicAdd("] and "atomicAdd(A.skipped, 1ull)" in wrench
    assert "for (" not in wrench and "while" not in wrench and "B.srec[4 * ga] =" not in wrench and not re.search(r"B\.\w+\[[^\]]+\] =[^=]", wrench)   # it reads state only
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 2
    assert not re.search(r"void k_batch_query_\w+\(", k) and "k_batch_rollout_act<" not in k and "k_batch_rollout_record<<<" not in k


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_use_no_scratch_and_spill_nothing():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_spring")
    assert set(rows) == {"k_batch_spring_wrench", "k_batch_spring_apply<false>", "k_batch_spring_apply<true>"}, sorted(rows)
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    for name, v in sorted(rows.items()):
        print(name, ": vgpr, sgpr, scratch, static lds, sgpr spills, vgpr spills =", v)
        assert v[2] == "0" and v[4] == "0" and v[5] == "0", (name, v)    # no scratch, no spills
        assert "`%s` %s / %s / 0 / 0 / 0" % (name, v[0], v[1]) in design, (name, v)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_marshals_a_rig_and_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self):
            self._h, self.n_worlds = None, 2

        def spring_count(self):
            return 4

    b, n = Handle(), 4
    for t in (torch.zeros((n, 12), dtype=torch.float64), torch.zeros((12, n), dtype=torch.float32).t(), torch.zeros((n - 1, 12), dtype=torch.float32),
              torch.zeros((n, 6), dtype=torch.float32)):
        with pytest.raises(ValueError) as e:
            b.apply_springs_dev(0.01, wrenches_out=t)
        assert "on cpu" not in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="on cpu"):
        b.apply_springs_dev(0.01, wrenches_out=torch.zeros((n, 12), dtype=torch.float32))
    with pytest.raises(mgf_amd.MgfError):                               # and a call whose arguments are all in order does reach C
        b.apply_springs_dev(0.01, wrenches_out=1 << 21)
    with pytest.raises(mgf_amd.MgfError):
        b.apply_springs(0.01, wrenches=True)
    with pytest.raises(mgf_amd.MgfError):                               # scalars and single rows for all; what reaches C is SPRING_DTYPE rows
        b.set_springs([0, 1, 1], [0, 1, 2], other=[1, -1, 0], pa=(0, 0, 0.5), pb=[(0, 0, 1), (0, 1, 0), (1, 0, 0)], rest=1.0, k=[1.0, 2.0, 3.0], c=0.1, lo=0.0)
    with pytest.raises(ValueError):
        b.set_springs([0, 1, 1], [0, 1], k=1.0)                         # neither one nor n
