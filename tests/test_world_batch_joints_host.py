"""The ball joints of a batch (mgf_batch_set_joints, mgf_batch_joint_count, mgf_batch_solve_joints, mgf_batch_solve_joints_dev) without a
GPU: the header, the library, the binding and the documents carry the calls, the record of 48 bytes and the three constants; the numpy
restatement (tests/batch_joint_cases.py) gives the fixed cases of the definition and holds against itself in float64; the plan is
items of one world with slots, ranks and degrees, and its dataflow gives the sequential order's bits whatever the schedule; what needs
no device is refused, in the header's order, with the rig unchanged; the launch sits between the actuation and the tick; and the
kernel has k_batch_solve's loop shape, no scratch and no spills."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_joint_cases as JC
from tests.util import ROOT, kernel_resources, read

f32 = np.float32
CALLS = ("mgf_batch_set_joints", "mgf_batch_joint_count", "mgf_batch_solve_joints", "mgf_batch_solve_joints_dev")
RIG_FILE = "host_batch_joint.inc"
H = f32(1.0 / 60.0)


def _seeded():
    lens = list(JC.LENGTHS)
    st = JC.synthetic_state(lens)
    rig, planted = JC.main_rig(lens, (st["x"] + st["delta"]).astype(f32))
    return lens, st, rig, planted


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls_the_record_and_the_constants():
    h = read("include", "mgf_hip.h")
    flat_h = re.sub(r"\s+", " ", h)
    for sig in ("MGF_API mgf_status mgf_batch_set_joints(mgf_batch* b, const mgf_batch_joint* j, int64_t n);",
                "MGF_API int64_t mgf_batch_joint_count(const mgf_batch* b);",
                "MGF_API mgf_status mgf_batch_solve_joints(mgf_batch* b, float h, int32_t iters, float* impulse_out);",
                "MGF_API mgf_status mgf_batch_solve_joints_dev(mgf_batch* b, float h, int32_t iters, float* impulse_out_dev);"):
        assert sig in flat_h, sig
    assert h.index("MGF_API mgf_status mgf_batch_apply_springs_dev(") < h.index("/* ---- ball joints between bodies") < h.index("/* name in {")
    consts = (("MGF_BATCH_JOINT_LAUNCHES", _capi.BATCH_JOINT_LAUNCHES, 1), ("MGF_BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK", _capi.BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK, 1),
              ("MGF_BATCH_MAX_WORLD_JOINTS", _capi.BATCH_MAX_WORLD_JOINTS, 256))
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for name, value, want in consts:
        m = re.search(r"#define %s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == value == want, name
        assert "pub const %s: i64 = %d;" % (name, want) in flat, name
        assert getattr(mgf_amd, name[4:]) is getattr(_capi, name[4:]), name
    section = h[h.index("/* ---- ball joints between bodies"):h.index("MGF_API mgf_status mgf_batch_solve_joints_dev(")]
    for word in ("ra = rotate(q_a, pa);  Pa = x_a + ra", "other == -1: rb = 0;  Pb = pb;  im_b = 0;  I_b = 0", "C = Pb - Pa;  s = beta / h;  bias = C * s",
                 "(e_k * im_a + cross(I_a * cross(ra, e_k), ra)) + (e_k * im_b + cross(I_b * cross(rb, e_k), rb))", "Kinv = invert(K)", "det == 0",
                 "Va = v_a + cross(omega_a, ra);  Vb = v_b + cross(omega_b, rb)", "P = Kinv * ((Vb - Va) + bias)",
                 "v_a = v_a + P * im_a;  omega_a = omega_a + I_a * cross(ra, P)", "Pn = -P;  v_b = v_b + Pn * im_b;  omega_b = omega_b + I_b * cross(rb, Pn)",
                 "acc_i = acc_i + P", "joints_skipped", "still takes its place in the order", "untouched to the bit", "no warm start", "several components",
                 "drive_launches", "rollout_launches", "the rig was not changed", "nothing enqueued", "mgf_batch_add_bodies", "no float atomic",
                 "mgf_batch_solve_joints_dev(b, dt, iters, NULL)", "ONCE", "mgf_batch_step itself stays World::step, launch for launch", "OUT OF SCOPE",
                 "coupled with the contacts", "limits and motors", "warm starting", "lone mgf_world", "inside mgf_batch_step", "impulses per tick",
                 "driven per tick"):
        assert word in section, word
    assert '"joints_skipped"' in h[h.index("/* name in {"):]
    # the record: 48 bytes, the same fields at the same offsets in the ctypes struct and the numpy dtype
    assert C.sizeof(_capi.BatchJoint) == 48 == _capi.JOINT_DTYPE.itemsize
    names = ["world", "body", "other", "flags", "pa", "beta", "pb", "pad"]
    assert [f[0] for f in _capi.BatchJoint._fields_] == list(_capi.JOINT_DTYPE.names) == names
    want_off = [0, 4, 8, 12, 16, 28, 32, 44]
    assert [_capi.JOINT_DTYPE.fields[k][1] for k in names] == want_off == [getattr(_capi.BatchJoint, k).offset for k in names]
    assert re.search(r"typedef struct mgf_batch_joint \{\s*int32_t world, body, other; uint32_t flags;[^\n]*\n\s*mgf_vec3 pa; float beta;[^\n]*\n\s*mgf_vec3 pb; float pad;[^\n]*\n"
                     r"\} mgf_batch_joint;", h)
    lib = mgf_amd.load_library()
    vp, i64, i32, fl = C.c_void_p, C.c_int64, C.c_int32, C.c_float
    want = {"mgf_batch_set_joints": (i32, [vp, vp, i64]), "mgf_batch_joint_count": (i64, [vp]),
            "mgf_batch_solve_joints": (i32, [vp, fl, i32, vp]), "mgf_batch_solve_joints_dev": (i32, [vp, fl, i32, vp])}
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == want[name], name
    for method in ("set_joints", "joint_count", "solve_joints", "solve_joints_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    assert mgf_amd.JOINT_DTYPE is _capi.JOINT_DTYPE
    for sig in ("pub fn mgf_batch_set_joints(b: *mut mgf_batch, j: *const mgf_batch_joint, n: i64) -> mgf_status;",
                "pub fn mgf_batch_joint_count(b: *const mgf_batch) -> i64;",
                "pub fn mgf_batch_solve_joints(b: *mut mgf_batch, h: f32, iters: i32, impulse_out: *mut f32) -> mgf_status;",
                "pub fn mgf_batch_solve_joints_dev(b: *mut mgf_batch, h: f32, iters: i32, impulse_out_dev: *mut f32) -> mgf_status;",
                "pub struct mgf_batch_joint { pub world: i32, pub body: i32, pub other: i32, pub flags: u32, pub pa: mgf_vec3, pub beta: f32, pub pb: mgf_vec3, pub pad: f32 }",
                "pub fn set_joints(", "pub fn joint_count(", "pub fn solve_joints(", "pub unsafe fn solve_joints_dev("):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_spring.h"') < kernels.index('#include "k_batch_joint.h"')
    assert "k_batch_joint_solve<GATED> (k_batch_joint.h)" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_spring.inc"') < hip.index('#include "%s"' % RIG_FILE)
    design = read("DESIGN.md")
    assert design.index("## Springs") < design.index("## Joints") < design.index("## 9.")
    sub = design[design.index("## Joints"):design.index("## Rollout touch traces")]
    for word in ("k_batch_joint_solve", "done[k] == t && act[k] == t", "Compiler output", "Out of scope", "batch_joint_bench.py", "MGF_BATCH_JOINT_LAUNCHES",
                 "MGF_BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK", "MGF_BATCH_MAX_WORLD_JOINTS", "__any", "kBatchSpinLimit", "bench.py", "Measured"):
        assert word in sub, word
    readme = read("README.md")
    assert "set_joints" in readme and "solve_joints_dev" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_joint_bench.py"))
    for text in (h, design):   # the earlier sections that listed joints as out of scope point here
        assert "ball joints since" in text


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def _two(xa, xb, qa=(1, 0, 0, 0), qb=(1, 0, 0, 0), va=(0, 0, 0), vb=(0, 0, 0), oa=(0, 0, 0), ob=(0, 0, 0), im=(1.0, 0.5), I=(4.0, 2.0)):
    eye = np.eye(3, dtype=f32).reshape(9)
    return {"x": f32([xa, xb]), "delta": np.zeros((2, 3), f32), "q": f32([qa, qb]), "v": f32([va, vb]), "omega": f32([oa, ob]),
            "inv_mass": f32(im), "inv_moment": f32([eye * I[0], eye * I[1]])}


def test_the_restatement_gives_the_fixed_cases_of_the_definition():
    # anchors at the centres, no gap: the relative velocity is removed in one sweep, momentum is kept, masses 1 and 2
    st = _two((0, 0, 0), (0, 0, 0), va=(3, 0, 0), vb=(0, 0, 0))
    v, om, acc, sk = JC.solve(JC.joint(0, 0, 1), H, 1, st, [2])
    assert not sk.any() and v.dtype == f32 and acc.dtype == f32
    assert np.allclose(v, [[1, 0, 0], [1, 0, 0]], atol=1e-6) and not om.any() and np.allclose(acc[0], [-2, 0, 0], atol=1e-6)   # P acts on `body`: it is braked
    # a world anchor with a gap and beta = 1: the point is sent to the anchor in one step - v = C / h
    st = _two((0, 0, 0), (5, 5, 5))
    v, om, acc, sk = JC.solve(JC.joint(0, 0, -1, pb=(0.5, 0, 0), beta=1.0), H, 1, st, [2])
    assert np.allclose(v[0], [30, 0, 0], rtol=1e-6) and not v[1].any() and not om.any() and not sk.any()
    # beta = 0 leaves the gap alone; iters = 0 does nothing
    v, om, acc, sk = JC.solve(JC.joint(0, 0, -1, pb=(0.5, 0, 0), beta=0.0), H, 3, st, [2])
    assert not v.any() and not acc.any()
    v, om, acc, sk = JC.solve(JC.joint(0, 0, -1, pb=(0.5, 0, 0), beta=1.0), H, 0, st, [2])
    assert not v.any() and not acc.any() and not sk.any()
    # an arm: the joint turns the body as well, and the anchor point's velocity, not the centre's, is what ends at rest
    st = _two((0, 0, 0), (0, 0, 0), va=(0, 2, 0), oa=(0, 0, 1))
    r = JC.joint(0, 0, -1, pa=(1, 0, 0), pb=(1, 0, 0))
    v, om, acc, sk = JC.solve(r, H, 1, st, [2])
    point = v[0].astype(np.float64) + np.cross(om[0].astype(np.float64), [1, 0, 0])
    assert np.abs(point).max() < 1e-6 and om[0, 2] != 1 and v[0, 1] != 2
    # one joint alone converges in one sweep: the second sweep's impulse is rounding
    a1 = JC.solve(r, H, 1, st, [2])[2]
    a2 = JC.solve(r, H, 2, st, [2])[2]
    assert np.abs(a2 - a1).max() < 1e-6 * np.abs(a1).max()
    # the skips: h = 0 with beta = 0 is 0 / 0, with beta > 0 an infinite bias; an arm that overflows; no velocity touched, a zero impulse
    st = _two((0, 0, 0), (2, 0, 0), va=(1, 2, 3), vb=(-1, 0, 1), oa=(1, 1, 1))
    for r, h in ((JC.joint(0, 0, 1, beta=0.0), 0.0), (JC.joint(0, 0, 1, beta=0.2), 0.0), (JC.joint(0, 0, 1, pa=(3e38, 0, 0)), H), (JC.joint(0, 1, -1, beta=0.0), 0.0)):
        v, om, acc, sk = JC.solve(r, h, 4, st, [2])
        assert sk.tolist() == [True] and not acc.any() and v.tobytes() == st["v"].tobytes() and om.tobytes() == st["omega"].tobytes()
    # a skipped joint keeps its place: the joints around it give what they give without it
    rig = np.concatenate([JC.joint(0, 0, 1, beta=0.2), JC.joint(0, 0, 1, pa=(3e38, 0, 0)), JC.joint(0, 1, -1, pb=(2, 1, 0), beta=0.2)])
    v3, om3, acc3, sk3 = JC.solve(rig, H, 4, st, [2])
    v2, om2, acc2, _ = JC.solve(rig[[0, 2]], H, 4, st, [2])
    assert sk3.tolist() == [False, True, False] and v3.tobytes() == v2.tobytes() and om3.tobytes() == om2.tobytes() and acc3[[0, 2]].tobytes() == acc2.tobytes()
    # worlds are independent, and the caller's interleaving does not matter: two worlds' joints in either interleaving
    st4 = {k: np.concatenate([a, a]) for k, a in st.items()}
    r0, r1 = JC.joint(0, 0, 1, pa=(0.1, 0, 0), beta=0.2), JC.joint(1, 1, 0, pb=(0, 0.2, 0), beta=0.1)
    va, oa, aa, _ = JC.solve(np.concatenate([r0, r1, r0]), H, 2, st4, [2, 2])
    vb, ob, ab, _ = JC.solve(np.concatenate([r0, r0, r1]), H, 2, st4, [2, 2])
    assert va.tobytes() == vb.tobytes() and oa.tobytes() == ob.tobytes() and aa[[0, 2, 1]].tobytes() == ab.tobytes()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
WORST_RESIDUAL = 2.91e-5   # measured: see the test below
RESIDUAL_BOUND = 8 * WORST_RESIDUAL


def test_the_definition_holds_against_itself_in_float64():
    """Every joint of the seeded rig (tests/batch_joint_cases.py: main_rig on synthetic_state, h = 1/60, beta = 0.2 and beta = 0) solved
    ALONE for one sweep in f32: the residual |(Vb - Va) + bias| of the f32 velocities, evaluated in float64 with the float64 run's own
    arms and bias, stays within a bound of the float64 run's residual.  The reference is the float64 restatement, never the library.
    Measured here on the CPU over the 2 x 276 joints that are not skipped: the worst f32 residual is 2.91e-5, at a joint whose bias is
    125 (2.3e-7 of it; the float64 run's residuals are below 1e-12) - WORST_RESIDUAL.  The bound allows 8 x that, 2.33e-4, for other
    seeds' rounding - RESIDUAL_BOUND."""
    lens, st, rig, planted = _seeded()
    worst, worst_bias, worst64 = 0.0, 0.0, 0.0
    for beta in (0.2, 0.0):
        rig["beta"] = beta
        J64 = JC.setup(rig, H, st, lens, np.float64)
        for i in range(len(rig)):
            v, om, acc, sk = JC.solve(rig[i:i + 1], H, 1, st, lens)
            v64, om64, _, sk64 = JC.solve(rig[i:i + 1], H, 1, st, lens, ft=np.float64)
            assert sk.tolist() == [i in planted] and not sk64.any()                      # (the planted arm overflows in f32 alone)
            if sk[0]:
                continue
            r32, r64 = JC.residual(J64[i], v, om), JC.residual(J64[i], v64, om64)
            if r32 > worst:
                worst, worst_bias = r32, float(np.linalg.norm(J64[i][4]))
            worst64 = max(worst64, r64)
            assert r32 <= r64 + RESIDUAL_BOUND, (i, beta, r32, r64)
    print("worst f32 residual", worst, "beside a bias of", worst_bias, "; worst f64 residual", worst64, "; bound", RESIDUAL_BOUND)
    assert worst64 < 1e-10


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_plan_is_items_of_one_world_with_slots_ranks_and_degrees():
    lens, st, rig, planted = _seeded()
    n = len(rig)
    assert n == 1 + 4 + 4 + 6 + 2 + 4 + JC.MAX and np.any(np.diff(rig["world"]) < 0)        # interleaved in the caller's array
    assert np.all(rig["body"] < np.int64(lens)[rig["world"]]) and np.all(rig["other"] < np.int64(lens)[rig["world"]]) and np.all(rig["other"] != rig["body"])
    items, joints, slots = JC.plan(rig)
    assert [it[0] for it in items] == [JC.ANCHOR, JC.CHAIN, JC.CHAIN_REV, JC.STAR, JC.HINGE, JC.RING, JC.FULL]     # no item for BARE and EMPTY
    assert [it[2] for it in items] == [1, 4, 4, 6, 2, 4, JC.MAX] and [it[3] for it in items] == [1, 5, 5, 7, 2, 4, 115]
    assert sorted(j[0] for j in joints) == list(range(n))
    for world, first, count, n_slots, first_slot in items:
        mine = joints[first:first + count]
        idx = [j[0] for j in mine]
        assert idx == sorted(idx) and np.all(rig["world"][idx] == world)                  # a world's joints stay in list order
        sl = slots[first_slot:first_slot + n_slots]
        assert len({b for b, _ in sl}) == n_slots == len(set(rig["body"][idx].tolist()) | set(rig["other"][idx][rig["other"][idx] >= 0].tolist()))
        seen = [0] * n_slots
        for i, sa, sb, ra, rb in mine:
            assert sl[sa][0] == rig["body"][i] and ra == seen[sa]
            seen[sa] += 1
            if rig["other"][i] >= 0:
                assert sl[sb][0] == rig["other"][i] and rb == seen[sb]
                seen[sb] += 1
            else:
                assert sb == -1
        assert seen == [d for _, d in sl] and min(seen) >= 1                             # a slot's degree: the joints that name its body
    star = items[3]
    assert max(d for _, d in slots[star[4]:star[4] + star[3]]) == 6                        # a chain of length 6 on one slot
    rev = joints[items[2][1]:items[2][1] + 4]
    assert [rig["body"][j[0]] for j in rev] == [3, 2, 1, 0]                                # the reversed chain: every dependency against the lane order
    full = joints[items[6][1]:items[6][1] + JC.MAX]
    slot_first = {}
    for lane, (i, sa, sb, ra, rb) in enumerate(full):
        for s in (sa, sb):
            if s >= 0:
                slot_first.setdefault(s, []).append(lane // 64)
    waves = [(w[k], w[k + 1]) for w in slot_first.values() for k in range(len(w) - 1)]
    assert set(lane // 64 for lane in range(JC.MAX)) == {0, 1, 2, 3} and any(a < b for a, b in waves)     # all four waves; dependencies cross them
    jointed = {b for b, _ in slots[items[6][4]:]}
    assert len(jointed) < JC.BIG and all(b not in jointed for b in range(101, JC.BIG, 2))  # bodies with no joint in between
    # the dataflow over ranks and degrees gives the sequential order's bits, whatever the schedule - and never stalls
    want = JC.solve(rig, H, 4, st, lens)
    for seed in (1, 2):
        got = JC.solve(rig, H, 4, st, lens, schedule=np.random.default_rng(seed))
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    assert np.flatnonzero(want[3]).tolist() == planted and not want[2][planted].any() and np.all(np.isfinite(want[0]))
    # the host's plan is that plan: a stable sort by world, slots in the order of first mention, reached behind every check
    src = read("mgf_amd", "csrc", RIG_FILE)
    plan = src[src.index("static void batch_joint_plan("):]
    plan = plan[:plan.index("\n}\n")]
    assert "std::stable_sort(" in plan and plan.index("std::stable_sort(") < plan.index("R.recs.assign(") < plan.index("R.stale = true;")
    assert plan.index("const auto a = slot(r.body);") < plan.index("r.other >= 0 ? slot(r.other)")
    assert "plan[4 * p + 1] = a.first | (b.first << 16);" in plan and "plan[4 * p + 2] = a.second | (b.second << 16);" in plan
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(", plan)
    lr = JC.late_joints([27, 18, 8])
    assert len(lr) == 24 and set(lr["world"].tolist()) == {0, 1, 2} and np.all(lr["other"] != lr["body"]) and np.all(lr["body"] < np.int64([27, 18, 8])[lr["world"]])


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_device_is_refused_in_the_headers_order_with_the_rig_unchanged():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced
    rig = np.zeros(4, _capi.JOINT_DTYPE)
    out = C.c_void_p(1 << 21)
    h = C.c_float(1.0 / 60.0)
    assert lib.mgf_batch_joint_count(None) == -1
    assert lib.mgf_batch_set_joints(None, rig.ctypes.data, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_joints(None, None, 0) == INV and "NULL" in err()
    assert lib.mgf_batch_set_joints(fake, None, 4) == INV and "NULL" in err()
    assert lib.mgf_batch_set_joints(fake, rig.ctypes.data, -1) == INV and "negative" in err()
    assert lib.mgf_batch_set_joints(fake, rig.ctypes.data, 1 << 31) == INV and "too many" in err()
    for fn in (lib.mgf_batch_solve_joints, lib.mgf_batch_solve_joints_dev):
        assert fn(None, h, 4, out) == INV and "NULL" in err()
        assert fn(None, C.c_float(np.nan), -1, None) == INV and "NULL" in err()             # the handle first
        for bad in (np.nan, np.inf, -np.inf):
            assert fn(fake, C.c_float(bad), -1, out) == INV and "h is not finite" in err(), bad   # h ahead of iters
        assert fn(fake, h, -1, out) == INV and "iters is negative" in err()
    src = read("mgf_amd", "csrc", RIG_FILE)
    body = src[src.index('extern "C" mgf_status mgf_batch_set_joints('):src.index('extern "C" int64_t mgf_batch_joint_count(')]
    plan_call = "batch_joint_plan(b->joints, j, n);"
    assert not re.search(r"b->joints\.|\bR\.", body.replace(plan_call, ""))                  # the rig changes in the plan step alone
    # (the two checks of `other`, with their two refusals, are the joint rigs' shared step: tests/test_world_batch_joint_family_host.py)
    marks = ["batch_rig_set_args(b, j, n_in)", 'batch_rig_ref_check(b, r.world, r.body, 0, "joint")', "batch_joint_other_check<JointKind>(b, r)",
             "r.flags != 0u || r.pad != 0.0f", "a joint's pa or pb is not finite: the rig was not changed",
             "a joint's beta is not in [0, 1]: the rig was not changed", "++per_world[(size_t)r.world] > MGF_BATCH_MAX_WORLD_JOINTS", plan_call]
    order = [body.index(s) for s in marks]
    assert order == sorted(order), order
    assert body.count("the rig was not changed") == 6 - 2
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(", body)                      # no device work at all
    # what tests/test_world_batch_rigs_host.py asks of a rig file: the shared steps used, not copied
    assert src.count("batch_rig_set_args(b, ") == 1 and src.count("batch_rig_up(b, R, ") == 1 and "batch_rig_up(b, R, T::word, 3)" in src and 'word = "joint";' in src
    for gone in ("BatchQueryPlan plan(", "batch_rig_upload(", "names a body its world does not hold", '"batch is NULL"'):
        assert gone not in src, gone
    host = read("mgf_amd", "csrc", "host_batch.inc")
    stale = host[host.index("static void batch_rigs_stale("):host.index('extern "C" mgf_status mgf_batch_add_bodies(')]
    assert host.count("BatchJointRig<mgf_batch_joint> joints;") == 1 and "b->joints.stale = true;" in stale
    assert '"joints_skipped"' in host[host.index('extern "C" mgf_status mgf_batch_counter('):]
    # the solve calls are one-line forwards to the joint rigs' shared steps, whose order - the refusals, the context, (device form) the
    # pointer looked up, and only then the first thing enqueued; one wait in the host form, a give-up reported behind it; one launch
    # behind batch_push and ready, counted once - tests/test_world_batch_joint_family_host.py holds; the ball joints have no table: row 0
    assert 'extern "C" mgf_status mgf_batch_solve_joints(mgf_batch* b, float h, int32_t iters, float* impulse_out) { return batch_joint_solve<JointKind>(b, h, iters, 0, impulse_out); }' in src
    dev = src[src.index('extern "C" mgf_status mgf_batch_solve_joints_dev('):]
    assert dev.count(";") == 1 and "return batch_joint_solve_dev<JointKind>(b, h, iters, 0, impulse_out_dev);" in dev
    kind = src[src.index("struct JointKind {"):src.index('extern "C" mgf_status mgf_batch_set_joints(')]
    assert "launches = MGF_BATCH_JOINT_LAUNCHES," in kind and "launch = k_batch_joint_solve<GATED>;" in kind and "table = false;" in kind and "using Rows = JointRows;" in kind
    assert "static constexpr uint32_t kWords = 3, kFloats = 3;" in read("mgf_amd", "csrc", "k_batch_joint.h")   # 12 bytes a joint of impulse
    assert "batch_single_parts(" not in src                                                   # joints read no shapes


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_launch_sits_between_the_actuation_and_the_tick_and_is_counted_once():
    host = read("mgf_amd", "csrc", "host_batch.inc")
    roll = read("mgf_amd", "csrc", "host_batch_rollout.inc")
    core = roll[roll.index("static mgf_status batch_rollout_run("):roll.index('extern "C" mgf_status mgf_batch_rollout_dev(')]
    assert "!b->joints.recs.empty()" in core and "!springs && !joints &&" in core           # the early return to the plain step sees the joint rig
    assert core.index("batch_push(") < core.index("batch_joint_hook<JointKind>(b, dt, iters, &H.joints)") < core.index("batch_step_run(b, dt, iters, n_ticks, stats, &H)")
    train = host[host.index("static mgf_status batch_step_run("):host.index('extern "C" mgf_status mgf_batch_step(')]
    tick = "batch_joint_tick<JointKind>(b, hook->joints, t, &hook->launches)"   # (the launch <true>, counted once by the kind's per_tick: tests/test_world_batch_joint_family_host.py)
    assert train.index("k_batch_spring_apply<true><<<") < train.index("k_batch_rollout_act<") < train.index(tick) < train.index("batch_collide(")
    assert train.count("batch_joint_tick<JointKind>") == 1 and "per_tick = MGF_BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK;" in read("mgf_amd", "csrc", RIG_FILE)
    # what the kernel reads of the handle is looked up again for every pass: inside the loop over the passes, ahead of the loop over the ticks
    assert train.index("for (uint32_t first = 0, pass = 0;") < train.index("batch_joint_pass<JointKind>(b, hook->joints);") < train.index("for (uint32_t t = first; t < NT; ++t)")
    # a give-up is the second error word, read back with the first
    assert "d2h(ctx, err, b->d_err.p, 2)" in train and "a lane of the joint solver gave up" in train
    step = host[host.index('extern "C" mgf_status mgf_batch_step('):host.index('extern "C" mgf_status mgf_batch_read_constraints(')]
    assert "batch_step_run(b, dt, iters, n_ticks, stats, nullptr)" in step and "joint" not in step   # mgf_batch_step applies no joint


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_kernel_has_the_batch_solvers_loop_shape_a_bounded_spin_and_no_float_atomic():
    k = read("mgf_amd", "csrc", "k_batch_joint.h")
    entry = k[k.index("void k_batch_joint_solve("):]
    assert entry[:entry.index("\n}\n")] == "void k_batch_joint_solve(BatchJointArgs A) {\n  batch_joint_loop<JointRows, GATED>(A);"
    # the kernel is one call of the joint solvers' skeleton: the loop shape is asserted of the skeleton (and again, for the three kernels
    # at once, in tests/test_world_batch_joint_family_host.py)
    loop_file = read("mgf_amd", "csrc", "k_batch_joint_loop.h")
    body = loop_file[loop_file.index("void batch_joint_loop("):]
    body = body[:body.index("\n}\n")]
    gate = "if (GATED && !(A.done[k] == A.tick && A.act[k] == A.tick)) return;"
    assert gate in body and body.index(gate) < body.index("__syncthreads()")                 # the workgroup's early return ahead of the first barrier
    assert body.count("__syncthreads()") == 2 and re.findall(r"atomic\w*\(", body.replace("__hip_atomic_load(", "").replace("__hip_atomic_store(", "")) == ["atomicAdd("]
    assert "atomicAdd(A.skipped, 1ull)" in body                                               # an integer count: no float atomic
    loop = body[body.index("while (open)"):body.index("if (s_fail != 0u) return;")]
    assert loop.count("__ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP") == 2 and loop.count("__ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP") == 2
    assert loop.index("if (!__any(ready)) __builtin_amdgcn_s_sleep(1);") < loop.index("if (ready) {") < loop.index("s_dyn[2 * sa] = ") < loop.index("__ATOMIC_RELEASE")
    assert "++spins > kBatchSpinLimit" in loop and "A.err[1] = 1u;" in loop and "A.err[0]" not in k
    assert "GATED" not in loop and "A.done" not in loop and "break" not in loop and "continue" not in loop and "return" not in loop
    back = body[body.index("if (s_fail != 0u) return;"):]
    assert "srec[4 * (size_t)body] = s_dyn[2 * s];" in back and "srec[4 * (size_t)body + 1] = s_dyn[2 * s + 1];" in back and "+ 2]" not in back   # words 0 and 1 alone
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 1
    assert not re.search(r"A\.act\[[^\]]+\] =[^=]", k) and not re.search(r"A\.done\[[^\]]+\] =[^=]", k)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernel_uses_no_scratch_and_spills_nothing():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_joint")
    assert set(rows) == {"k_batch_joint_solve<false>", "k_batch_joint_solve<true>"}, sorted(rows)
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    for name, v in sorted(rows.items()):
        print(name, ": vgpr, sgpr, scratch, static lds, sgpr spills, vgpr spills =", v)
        assert v[2] == "0" and v[4] == "0" and v[5] == "0", (name, v)    # no scratch, no spills
        assert int(v[3]) <= 16, (name, v)                                 # static LDS: the give-up flag alone
        assert "`%s` %s / %s / %s / 0 / 0" % (name, v[0], v[1], v[3]) in design, (name, v)


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_marshals_a_rig_and_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self):
            self._h, self.n_worlds = None, 2

        def joint_count(self):
            return 4

    b, n = Handle(), 4
    for t in (torch.zeros((n, 3), dtype=torch.float64), torch.zeros((3, n), dtype=torch.float32).t(), torch.zeros((n - 1, 3), dtype=torch.float32),
              torch.zeros((n, 12), dtype=torch.float32)):
        with pytest.raises(ValueError) as e:
            b.solve_joints_dev(0.01, 4, impulses_dev=t)
        assert "on cpu" not in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="on cpu"):
        b.solve_joints_dev(0.01, 4, impulses_dev=torch.zeros((n, 3), dtype=torch.float32))
    with pytest.raises(mgf_amd.MgfError):                               # and a call whose arguments are all in order does reach C
        b.solve_joints_dev(0.01, 4, impulses_dev=1 << 21)
    with pytest.raises(mgf_amd.MgfError):
        b.solve_joints(0.01, 4, impulses=True)
    with pytest.raises(mgf_amd.MgfError):                               # scalars and single rows for all; what reaches C is JOINT_DTYPE rows
        b.set_joints([0, 1, 1], [0, 1, 2], other=[1, -1, 0], pa=(0, 0, 0.5), pb=[(0, 0, 1), (0, 1, 0), (1, 0, 0)], beta=0.2)
    with pytest.raises(ValueError):
        b.set_joints([0, 1, 1], [0, 1])                                 # neither one nor n
