"""The contact sensors of a batch (mgf_batch_set_touches, mgf_batch_touch_count, mgf_batch_read_touches, mgf_batch_read_touches_dev)
without a GPU: the header, the library, the binding and the documents carry the four calls; what can be refused before a device is
looked at is refused there, before the handle is dereferenced, and the device form looks its pointer up before it enqueues anything; the
binding turns a wrong tensor down before it calls C; the kernel uses no scratch, spills nothing and keeps the figures DESIGN.md records;
the inputs of the GPU tests (tests/batch_touch_cases.py) are not trivial, shown by the oracle alone; and the restated fold agrees with
tests/batch_observe_cases.fold wherever the two definitions meet."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_observe_cases as OC
from tests import batch_parts_cases as PC
from tests import batch_query_cases as BQ
from tests import batch_touch_cases as TC
from tests.util import ROOT, kernel_resources, oracle_world, read

CALLS = ("mgf_batch_set_touches", "mgf_batch_touch_count", "mgf_batch_read_touches", "mgf_batch_read_touches_dev")
ANY, ANY_BODY, STATIC, FRAME = _capi.TOUCH_ANY, _capi.TOUCH_ANY_BODY, _capi.TOUCH_STATIC, _capi.TOUCH_BODY_FRAME


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_documents_carry_the_calls():
    h = read("include", "mgf_hip.h")
    for sig in (r"MGF_API mgf_status mgf_batch_set_touches\(mgf_batch\* b, const mgf_batch_touch\* t, int64_t n\);",
                r"MGF_API int64_t +mgf_batch_touch_count\(const mgf_batch\* b\);",
                r"MGF_API mgf_status mgf_batch_read_touches\(mgf_batch\* b, mgf_touch_report\* out, int64_t cap\);",
                r"MGF_API mgf_status mgf_batch_read_touches_dev\(mgf_batch\* b, mgf_touch_report\* out_dev, int64_t cap\);"):
        assert re.search(sig, h), sig
    assert "typedef struct mgf_batch_touch { int32_t world, body, other, flags; } mgf_batch_touch;" in h
    assert re.search(r"typedef struct mgf_touch_report \{\s*int32_t n_contacts, partner, record, reserved0;\s*mgf_vec3 impulse;\s+float normal_impulse;\s*"
                     r"mgf_vec3 push;\s+float strongest_impulse;\s*mgf_vec3 arm;\s+float reserved1;\s*\} mgf_touch_report;", h)
    for name, value in (("MGF_TOUCH_STATIC", _capi.TOUCH_STATIC), ("MGF_TOUCH_ANY_BODY", _capi.TOUCH_ANY_BODY), ("MGF_TOUCH_ANY", _capi.TOUCH_ANY),
                        ("MGF_TOUCH_NONE", _capi.TOUCH_NONE), ("MGF_TOUCH_BODY_FRAME", _capi.TOUCH_BODY_FRAME), ("MGF_BATCH_TOUCH_LAUNCHES", _capi.BATCH_TOUCH_LAUNCHES)):
        m = re.search(r"#define %s +\(?(-?\d+)\)?" % name, h)
        assert m and int(m.group(1)) == value, name
    assert (_capi.TOUCH_STATIC, _capi.TOUCH_ANY_BODY, _capi.TOUCH_ANY, _capi.TOUCH_NONE, _capi.TOUCH_BODY_FRAME, _capi.BATCH_TOUCH_LAUNCHES) == (-1, -2, -3, -4, 1, 1)
    assert _capi.TOUCH_DTYPE.itemsize == 16 and _capi.TOUCH_REPORT_DTYPE.itemsize == 64
    assert _capi.TOUCH_DTYPE.names == ("world", "body", "other", "flags")
    assert [(_capi.TOUCH_REPORT_DTYPE.fields[f][1]) for f in ("n_contacts", "partner", "record", "reserved0", "impulse", "normal_impulse", "push",
                                                               "strongest_impulse", "arm", "reserved1")] == [0, 4, 8, 12, 16, 28, 32, 44, 48, 60]
    for name in ("TOUCH_DTYPE", "TOUCH_REPORT_DTYPE", "TOUCH_STATIC", "TOUCH_ANY_BODY", "TOUCH_ANY", "TOUCH_NONE", "TOUCH_BODY_FRAME", "BATCH_TOUCH_LAUNCHES"):
        assert getattr(mgf_amd, name) is getattr(_capi, name) or getattr(mgf_amd, name) == getattr(_capi, name), name
    # the section: behind the zones' nearest-first reads, ahead of mgf_batch_counter
    assert (h.index("mgf_batch_overlap_nearest_dev(") < h.index("---- contact sensors:") < h.index("#define MGF_TOUCH_STATIC") < h.index("mgf_batch_set_touches(")
            < h.index("mgf_batch_read_touches_dev(mgf_batch* b") < h.index("MGF_API mgf_status mgf_batch_counter("))
    section = re.sub(r"\s*\n \* ", " ", h[h.index("---- contact sensors:"):h.index("MGF_API mgf_status mgf_batch_counter(")])
    for word in ("mgf_batch_read_constraints(world)", "empty before the first tick", "unchanged by mgf_batch_write_state", "a == x in ascending list index",
                 "b == x in ascending list index", "solver.rs:203-252", "-1 for RigidBodyRef::Static", "MGF_TOUCH_ANY_BODY: the partner is >= 0",
                 "impulse = impulse - t", "impulse = impulse + t", "no fused multiply-add", "mgf_body_contacts bit for bit", "equals its n_terrain",
                 "ties and NaN keep the earlier record", "every sign bit flipped", "arm is ra where x is `a` and rb where x is `b`",
                 "rotate((q.s, -q.x, -q.y, -q.z), v)", "AT ONCE", "partner = MGF_TOUCH_NONE, record = -1", "always 0", "depends on its sensor and its world only",
                 "bit-identical", "mgf_batch_copy_worlds(_where) carries the list", "MGF_BATCH_TOUCH_LAUNCHES = 1", "no collider gather",
                 "several components", "OUT OF SCOPE", "tangent impulses", "the k strongest contacts", "hipGraph capture", "other < -3", "other == body",
                 "a flag bit beyond MGF_TOUCH_BODY_FRAME", "MGF_ERR_CAPACITY", "nothing enqueued", "64 count bytes, aligned to 4 bytes"):
        assert word in section, word
    lib = mgf_amd.load_library()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    want = {"mgf_batch_set_touches": (i32, [vp, vp, i64]), "mgf_batch_touch_count": (i64, [vp]), "mgf_batch_read_touches": (i32, [vp, vp, i64]),
            "mgf_batch_read_touches_dev": (i32, [vp, vp, i64])}
    for name in CALLS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == want[name], name
    for method in ("set_touches", "touch_count", "read_touches", "read_touches_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for sig in ("pub fn mgf_batch_set_touches(b: *mut mgf_batch, t: *const mgf_batch_touch, n: i64) -> mgf_status;",
                "pub fn mgf_batch_touch_count(b: *const mgf_batch) -> i64;",
                "pub fn mgf_batch_read_touches(b: *mut mgf_batch, out: *mut mgf_touch_report, cap: i64) -> mgf_status;",
                "pub fn mgf_batch_read_touches_dev(b: *mut mgf_batch, out_dev: *mut mgf_touch_report, cap: i64) -> mgf_status;",
                "pub struct mgf_batch_touch { pub world: i32, pub body: i32, pub other: i32, pub flags: i32 }",
                "pub struct mgf_touch_report { pub n_contacts: i32, pub partner: i32, pub record: i32, pub reserved0: i32, pub impulse: mgf_vec3, "
                "pub normal_impulse: f32, pub push: mgf_vec3, pub strongest_impulse: f32, pub arm: mgf_vec3, pub reserved1: f32 }"):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert kernels.index('#include "k_batch_nearest.h"') < kernels.index('#include "k_batch_touch.h"') and "k_batch_touch (k_batch_touch.h)" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_nearest.inc"') < hip.index('#include "host_batch_touch.inc"')
    host = read("mgf_amd", "csrc", "host_batch.inc")
    assert host.count("BatchRig<mgf_batch_touch> touches;") == 1 and "b->touches.stale = true;" in host[host.index("static void batch_rigs_stale("):][:400]
    design = read("DESIGN.md")
    sub = design[design.index("### Contact sensors"):design.index("## 9. Limits")]
    for word in ("k_batch_touch", "Definition", "Compiler output", "Measured", "batch_touch_bench.py", "Out of scope"):
        assert word in sub, word
    readme = read("README.md")
    for word in ("set_touches", "read_touches", "read_touches_dev"):
        assert word in readme, word
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_touch_bench.py"))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
ENQUEUE = r"batch_touch_run\(|batch_rig_up\(|batch_rig_upload\(|batch_push\(|hipMemsetAsync|hipMemcpyAsync|<<<|\.ensure\(|h2d\("


def test_what_needs_no_device_is_refused_before_the_handle_is_dereferenced():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced; addresses that are never looked up
    recs, out = C.c_void_p(1 << 20), C.c_void_p(1 << 21)
    fn = lib.mgf_batch_set_touches
    assert fn(None, recs, 4) == INV and "batch is NULL" in err()
    assert fn(None, None, 0) == INV and "batch is NULL" in err()
    assert fn(fake, recs, -1) == INV and "negative" in err()
    assert fn(fake, None, -(1 << 40)) == INV and "negative" in err()
    assert fn(fake, recs, 1 << 31) == INV and "too many" in err()
    assert fn(fake, None, 1 << 31) == INV and "too many" in err()            # n ahead of the NULL array
    assert fn(fake, None, 4) == INV and "NULL argument" in err()
    assert lib.mgf_batch_touch_count(None) == -1
    for fn in (lib.mgf_batch_read_touches, lib.mgf_batch_read_touches_dev):
        assert fn(None, out, 4) == INV and "batch is NULL" in err()
        assert fn(None, None, -1) == INV and "batch is NULL" in err()       # the handle ahead of the cap
        assert fn(fake, out, -1) == INV and "negative" in err()
        assert fn(fake, None, -(1 << 40)) == INV and "negative" in err()    # the cap ahead of a NULL out
    # what needs the handle comes behind these and ahead of any device work (read here; run in tests/test_gpu_world_batch_touches.py)
    src = read("mgf_amd", "csrc", "host_batch_touch.inc")
    args = src[src.index("static mgf_status batch_touch_read_args("):src.index('extern "C" mgf_status mgf_batch_read_touches(')]
    assert args.index("batch_rig_handle(b)") < args.index("batch_rig_cap(cap)") < args.index("b->touches.recs.size()") < args.index("batch_rig_fits(*n, cap, out != nullptr)")
    assert args.index("b->") > args.index("batch_rig_cap(cap)")               # nothing of the handle is read before them
    # the set call: every record checked, in the header's order, before the first change of the rig; no device work at all
    body = src[src.index('extern "C" mgf_status mgf_batch_set_touches('):src.index('extern "C" int64_t mgf_batch_touch_count(')]
    assert (body.index("batch_rig_set_args(b, t, n_in)") < body.index('batch_rig_ref_check(b, t[i].world, t[i].body, 0, "contact sensor")')
            < body.index("t[i].other < MGF_TOUCH_ANY") < body.index("t[i].other == t[i].body") < body.index("t[i].flags & ~MGF_TOUCH_BODY_FRAME")
            < body.index("batch_rig_plan(b, R, t, n);"))
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(|ctx_bind", body)
    # neither read goes through batch_single_parts: a batch with bodies of several components is answered
    assert "batch_single_parts(" not in src.replace("(no batch_single_parts)", "")
    # the device form: the pointer looked up before the first enqueue; an empty rig enqueues nothing; no wait, no copy
    run = src[src.index('extern "C" mgf_status mgf_batch_read_touches_dev('):]
    first_enqueue = min(m.start() for m in re.finditer(ENQUEUE, run))
    assert run.index("batch_touch_read_args(") < run.index("ctx_bind(") < run.index('dev_span(b->ctx, out_dev, 64 * n, "out_dev")') < run.index("batch_call_begin(b)")
    assert run.index("dev_span(") < run.index("if (n == 0) return MGF_OK;") < first_enqueue
    assert "hipStreamSynchronize" not in run and "hipMemcpy" not in run
    helper = src[src.index("static mgf_status batch_touch_run("):src.index("// the refusals of both read calls")]
    assert helper.count("<<<") == 1 and "k_batch_touch<<<" in helper and "hipStreamSynchronize" not in helper and "hipMemcpy" not in helper
    assert "batch_cols_refresh" not in src                                     # no collider gather: nothing here reads a shape
    assert helper.index("batch_push(") < helper.index('batch_rig_up(b, R, "contact sensor", 3)') < helper.index("k_batch_touch<<<")
    assert helper.index("LAUNCH_CHECK();") < helper.index("b->q_launches += MGF_BATCH_TOUCH_LAUNCHES;")
    assert src.count("<<<") == 1 and src.count("b->q_launches += MGF_BATCH_TOUCH_LAUNCHES;") == 1
    host = src[src.index('extern "C" mgf_status mgf_batch_read_touches('):src.index('extern "C" mgf_status mgf_batch_read_touches_dev(')]
    assert host.count("hipMemcpyAsync(") == 1 and host.count("hipStreamSynchronize(") == 1 and host.index("if (n == 0) return MGF_OK;") < host.index(".ensure(")
    # the kernel: nothing built in global memory, no atomic, no float atomic, no exit, no assembly; barriers in the tile loop alone
    k = read("mgf_amd", "csrc", "k_batch_touch.h")
    code = re.sub(r"//[^\n]*", "", k[k.index("#pragma once"):])
    assert not re.search(r"atomic|\brows\b|return;|break;|continue;|\basm\b|__shfl|__ballot|\bfmaf?\(|__fm", code)
    assert code.count("__syncthreads()") == 2 and "__shared__" not in code.replace("extern __shared__ float4 s_dyn[];", "")
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 1
    assert re.findall(r"\bo\[(\d)\] = TouchWord\{", code) == ["0", "1", "2", "3"]
    assert "A.out" not in code.replace("TouchWord* o = A.out + 4 * (size_t)qi;", "")       # the only global store: a report's four words of 16 bytes


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self):
            self._h, self.n_worlds = None, 2

        def touch_count(self):
            return 4

    b, n = Handle(), 4
    for t in (torch.zeros((n, 16), dtype=torch.float64), torch.zeros((n, 16), dtype=torch.int64), torch.zeros((n, 16), dtype=torch.int16),
              torch.zeros((16, n), dtype=torch.int32).t(), torch.zeros((n - 1, 16), dtype=torch.int32), torch.zeros((n, 15), dtype=torch.float32),
              torch.zeros(n * 16, dtype=torch.int32), torch.zeros((n, 0), dtype=torch.int32)):
        with pytest.raises(ValueError) as e:
            b.read_touches_dev(t)
        assert "on cpu" not in str(e.value), str(e.value)              # turned down for what it is, not for where it is
    for dtype in (torch.int32, torch.float32):
        with pytest.raises(ValueError, match="on cpu"):                 # everything right but the device
            b.read_touches_dev(torch.zeros((n, 16), dtype=dtype))
    with pytest.raises(ValueError, match="required"):
        b.read_touches_dev(None)
    with pytest.raises(ValueError, match="required"):
        b.set_touches(0)
    with pytest.raises(mgf_amd.MgfError):                               # and a call whose arguments are all in order does reach C
        b.read_touches_dev(1 << 20)
    with pytest.raises(mgf_amd.MgfError):
        b.read_touches()
    with pytest.raises(mgf_amd.MgfError):
        b.set_touches([0, 1], body=[3, 4], other=ANY, body_frame=[False, True])
    with pytest.raises(mgf_amd.MgfError):
        b.set_touches(np.zeros(3, mgf_amd.TOUCH_DTYPE))
    # the rows the keyword form builds: scalars for all, the flag from body_frame
    rows = _capi._rig_rows(_capi.TOUCH_DTYPE, world=[0, 1, 1], body=[3, 4, 5], other=STATIC, flags=np.where(np.asarray([False, True, False]), FRAME, 0))
    assert rows.tolist() == [(0, 3, STATIC, 0), (1, 4, STATIC, FRAME), (1, 5, STATIC, 0)]


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_kernel_uses_no_scratch_spills_nothing_and_keeps_the_figures_the_design_records():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_touch")
    assert set(rows) == {"k_batch_touch"}, sorted(rows)
    design = re.sub(r"\s+", " ", read("DESIGN.md"))
    for name, v in rows.items():
        assert (v[2], v[3], v[4], v[5]) == ("0", "0", "0", "0"), (name, v)       # no scratch, no static LDS, no spills
        assert int(v[0]) <= 64, (name, v)                                         # eight waves a SIMD at 64 VGPRs
        assert f"`{name}` {v[0]} / {v[1]} / 0 / 0 / 0" in design, (name, v)       # the line DESIGN.md records
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_lane_masks.py")], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 lane masks" in r.stdout, r.stdout[-400:]


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def _at(sc, ticks, ow=None):
    ow = oracle_world(sc) if ow is None else ow
    for _ in range(ticks):
        ow.step(float(sc["dt"]), sc["iters"])
    return ow.constraints(), ow.state()["q"]


@pytest.fixture(scope="module")
def inputs():
    """the oracle's lists and rows q: the piles at tick 30, the capsules at tick 20, the bodies of several components at TC.PARTS_TICK"""
    piles = BQ.pile_scenes()
    caps = OC.capsule_scenes()
    parts = PC.six_scenes()
    return dict(piles=(piles, [_at(sc, 30) for sc in piles]), caps=(caps, [_at(sc, 20) for sc in caps]),
                parts=(parts, [_at(sc, TC.PARTS_TICK, ow) for sc, ow in zip(parts, PC.oracles(parts))]))


def test_the_piles_hold_what_the_issue_counted_by_the_oracle_alone(inputs):
    scs, at = inputs["piles"]
    for k, records, static, both, late in ((TC.SMALL, 157, 16, 46, 51), (TC.MID, 952, 64, 296, 305)):
        cons, q = at[k]
        n = len(scs[k]["comps"])
        own, asb = TC.roles(cons, n)
        assert (len(cons), int(np.sum(cons["b"] < 0))) == (records, static)
        assert sum(1 for x in range(n) if own[x] and asb[x]) == both
        assert sum(1 for x in range(n) if TC.strongest_is_late(cons, x)) == late
        assert not np.any(np.all(q == np.float32([1, 0, 0, 0]), axis=1))         # every body's q away from identity
        assert np.any(cons["normal_impulse"] == 0)
        # what the kernel uses of a list, and what it does not need: ascending in `a`; for body pairs b < a
        assert np.all(np.diff(cons["a"]) >= 0) and np.all(cons["b"] < cons["a"])


def test_the_layouts_hold_the_cases_the_gpu_tests_rely_on(inputs):
    kinds = {k: [] for k in TC.KINDS}
    seen = dict(both=0, late=0, low=0, high=0, two_filters=0, twice=0, framed=0)
    for name, skip in (("piles", (TC.NO_SENSOR_WORLD,)), ("caps", ()), ("parts", ())):
        scs, at = inputs[name]
        lengths = [PC.n_bodies(sc) for sc in scs]
        lists, qs = [c for c, _ in at], [q for _, q in at]
        rig = TC.rig_of(lists, lengths, skip=skip)
        assert len(rig) and set(rig["world"].tolist()) == {k for k in range(len(scs)) if lengths[k] and k not in skip}
        assert np.any(np.diff(rig["world"]) < 0)                                  # sensors in mixed world order
        for k, v in TC.summary(rig, lists).items():
            kinds[k] += v
        reports = TC.fold_rig(rig, lists, qs)
        plain = rig.copy()
        plain["flags"] = 0
        unrotated = TC.fold_rig(plain, lists, qs)
        for i, s in enumerate(rig):
            ch = TC.chain(lists[int(s["world"])], int(s["body"]), int(s["other"]))
            roles = {is_a for _, is_a, _ in ch}
            seen["both"] += roles == {True, False}
            seen["late"] += bool(ch) and reports["record"][i] != ch[0][0]
            seen["low"] += bool(ch) and 0 <= s["other"] < s["body"]
            seen["high"] += bool(ch) and s["other"] > s["body"]
            seen["framed"] += bool(s["flags"]) and all(reports[f][i].tobytes() != unrotated[f][i].tobytes() for f in ("impulse", "push", "arm"))
        uniq, counts = np.unique(rig, return_counts=True)
        seen["twice"] += int(np.sum(counts > 1))
        on = {}
        for s in rig:
            on.setdefault((int(s["world"]), int(s["body"])), set()).add(int(s["other"]))
        seen["two_filters"] += sum(1 for v in on.values() if len(v) > 1)
    for k, v in kinds.items():
        assert any(m >= 2 for m in v) and any(m == 0 for m in v) and any(m == 1 for m in v), k
    assert all(v > 0 for v in seen.values()), seen
    # more sensors on one world than a work item holds
    scs, at = inputs["piles"]
    for count in (257, 600):
        rig = TC.many_on_one_world(at[TC.SMALL][0], 96, TC.SMALL, count)
        assert len(rig) == count and np.all(rig["world"] == TC.SMALL) and len(np.unique(rig)) > 256
    # the manifolds of the bodies of several components: a pair of bodies with several consecutive records
    scs, at = inputs["parts"]
    assert PC.largest_manifold(at[PC.DUMBBELLS][0]) >= 2 and PC.largest_manifold(at[PC.JACKS][0]) >= 2


def test_fold_touch_with_any_is_the_per_body_fold(inputs):
    for name in ("piles", "caps", "parts"):
        scs, at = inputs[name]
        for k, (cons, q) in enumerate(at):
            n = PC.n_bodies(scs[k])
            want = OC.fold(cons, n)
            rig = np.zeros(2 * n, mgf_amd.TOUCH_DTYPE)
            rig["body"], rig["other"] = np.tile(np.arange(n), 2), np.repeat([ANY, STATIC], n)
            got = TC.fold_rig(rig, {0: cons}, {0: q})
            for f in ("n_contacts", "impulse", "normal_impulse"):
                assert np.ascontiguousarray(got[f][:n]).tobytes() == np.ascontiguousarray(want[f]).tobytes(), (name, k, f)
            assert got["n_contacts"][n:].tolist() == want["n_terrain"].tolist(), (name, k)
            touched = got["n_contacts"][:n] > 0
            assert np.all(got["partner"][:n][~touched] == _capi.TOUCH_NONE) and np.all(got["record"][:n][~touched] == -1)
            strongest = np.float32([max((cons["normal_impulse"][c] for c, _, _ in TC.chain(cons, x, ANY)), default=0.0) for x in range(n)])
            assert got["strongest_impulse"][:n].tobytes() == strongest.tobytes(), (name, k)
    # the definition's corners on a list of four records written by hand: a tie keeps the earlier record, the push of `a` is the normal's
    # sign bits flipped (a zero becomes -0), the frame turns the three vectors and nothing else
    cons = np.zeros(4, _capi.CONSTRAINT_DTYPE)
    cons["a"], cons["b"] = [1, 2, 2, 3], [-1, 1, 1, 2]
    cons["normal"] = [(0, 1, 0), (1, 0, 0), (0, 0, 1), (0, 1, 0)]
    cons["normal_impulse"] = [2.0, 3.0, 3.0, 0.5]
    cons["ra"], cons["rb"] = np.arange(12).reshape(4, 3) + 1, -(np.arange(12).reshape(4, 3) + 1)
    half = np.float32(np.sqrt(0.5))
    q = np.float32([[1, 0, 0, 0], [1, 0, 0, 0], [half, 0, 0, half], [1, 0, 0, 0]])      # body 2: a quarter turn about z
    one = lambda body, other, flags=0: TC.fold_touch(cons, q, np.array([(0, body, other, flags)], mgf_amd.TOUCH_DTYPE)[0])
    r = one(2, 1)
    assert (r["n_contacts"], r["partner"], r["record"]) == (2, 1, 1) and r["impulse"].tolist() == [-3.0, 0.0, -3.0] and r["normal_impulse"] == 6.0
    assert r["push"].view(np.uint32).tolist() == [0xBF800000, 0x80000000, 0x80000000] and r["arm"].tolist() == [4.0, 5.0, 6.0]
    r = one(1, 2)
    assert (r["n_contacts"], r["record"]) == (2, 1) and r["impulse"].tolist() == [3.0, 0.0, 3.0] and r["push"].tolist() == [1.0, 0.0, 0.0] and r["arm"].tolist() == [-4.0, -5.0, -6.0]
    r = one(1, ANY)
    assert (r["n_contacts"], r["partner"], r["record"], float(r["strongest_impulse"])) == (3, 2, 1, 3.0) and r["impulse"].tolist() == [3.0, -2.0, 3.0]
    assert one(1, STATIC)["n_contacts"] == 1 and one(1, ANY_BODY)["n_contacts"] == 2 and one(0, ANY)["partner"] == _capi.TOUCH_NONE
    assert one(0, ANY, FRAME).tobytes() == one(0, ANY).tobytes()
    w, f = one(2, ANY), one(2, ANY, FRAME)
    assert (w["n_contacts"], w["record"], w["partner"]) == (3, 1, 1) and w["impulse"].tolist() == [-3.0, 0.5, -3.0]
    assert np.allclose(f["impulse"], [0.5, 3.0, -3.0], atol=1e-6) and np.allclose(f["push"], [0.0, 1.0, 0.0], atol=1e-6)
    for name in ("n_contacts", "partner", "record", "normal_impulse", "strongest_impulse"):
        assert w[name] == f[name], name
