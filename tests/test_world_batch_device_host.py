"""The device-pointer calls of a batch (mgf_batch_gather_state_dev, _set_many_dev, _set_forces_dev, _apply_impulses_dev,
_read_body_contacts_dev, _copy_worlds_where, mgf_ctx_synchronize) without a GPU: the header declares them, the library, the Python
binding and INTEGRATION.md carry them, what can be refused before a device is looked at is refused there, the binding turns down a
tensor of the wrong kind before it calls C, the new kernels use no scratch memory, spill nothing and pass the lane-mask check - and the
inputs of the GPU tests are what those tests need, by numpy and the oracle alone."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_device_cases as DV
from tests.util import ROOT, kernel_resources, oracle_world, read

SET = r"mgf_batch\* b, const int32_t\* body_dev, int64_t n, "
ENTRY_POINTS = {
    "mgf_ctx_synchronize": r"mgf_status mgf_ctx_synchronize\(mgf_ctx\* ctx\);",
    "mgf_batch_gather_state_dev": r"mgf_status mgf_batch_gather_state_dev\(mgf_batch\* b, const int32_t\* body_dev, int64_t n,\s*"
                                  r"float\* x, float\* q, float\* v, float\* omega, float\* force, float\* torque\);",
    "mgf_batch_set_many_dev": r"mgf_status mgf_batch_set_many_dev\(" + SET + r"const float\* linear, const float\* angular\);",
    "mgf_batch_set_forces_dev": r"mgf_status mgf_batch_set_forces_dev\(" + SET + r"const float\* force, const float\* torque\);",
    "mgf_batch_apply_impulses_dev": r"mgf_status mgf_batch_apply_impulses_dev\(" + SET + r"const float\* linear, const float\* angular\);",
    "mgf_batch_read_body_contacts_dev": r"mgf_status mgf_batch_read_body_contacts_dev\(mgf_batch\* b, int64_t world, mgf_body_contacts\* out_dev, int64_t cap\);",
    "mgf_batch_copy_worlds_where": r"mgf_status mgf_batch_copy_worlds_where\(mgf_batch\* dst, const int32_t\* dst_world, const mgf_batch\* src, "
                                   r"const int32_t\* src_world,\s*int64_t n, const int32_t\* mask_dev\);",
}
NEW_KERNELS = {"k_batch_dev_gather", "k_batch_dev_count", "k_batch_dev_fill", "k_batch_dev_copy_where"} | {
    f"k_batch_dev_apply<{mode}, {seg}>" for mode in (0, 1, 2) for seg in ("false", "true")}


def test_header_declares_the_calls_the_launch_constant_and_what_is_left_out():
    h = read("include", "mgf_hip.h")
    for name, sig in ENTRY_POINTS.items():
        assert re.search(r"MGF_API " + sig, h), name
    section = h[h.index("device-pointer calls"):]
    m = re.search(r"#define MGF_BATCH_DEV_SET_LAUNCHES (\d+)", section)
    assert m and int(m.group(1)) == _capi.BATCH_DEV_SET_LAUNCHES
    for word in ("device_skipped", "pair_table_uploads", "drive_launches", "hipPointerGetAttributes", "hipMemGetAddressRange", "nothing enqueued",
                 "skipped whole", "highest array index", "ascending array index", "no float atomic", "OUT OF SCOPE", "rays, sweeps and box queries",
                 "hipGraph", "lone mgf_world", "RETURNS WITHOUT WAITING"):
        assert word in section, word
    design = read("DESIGN.md")
    sub = design[design.index("Device-pointer calls"):]
    for word in ("k_batch_dev_apply", "insertion", "device_skipped", "hipGraph", "batch_device_bench.py"):
        assert word in sub, word
    assert "gather_state" in read("README.md") and "copy_worlds_where" in read("README.md")
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert "k_batch_dev.h" in kernels and "k_batch_dev_gather" in kernels
    assert '#include "host_batch_dev.inc"' in read("mgf_amd", "csrc", "mgf_hip.hip")


def test_library_and_binding_export_them_with_their_signatures():
    lib = mgf_amd.load_library()
    vp, i64 = C.c_void_p, C.c_int64
    want = {
        "mgf_ctx_synchronize": [vp],
        "mgf_batch_gather_state_dev": [vp, vp, i64, vp, vp, vp, vp, vp, vp],
        "mgf_batch_set_many_dev": [vp, vp, i64, vp, vp],
        "mgf_batch_set_forces_dev": [vp, vp, i64, vp, vp],
        "mgf_batch_apply_impulses_dev": [vp, vp, i64, vp, vp],
        "mgf_batch_read_body_contacts_dev": [vp, i64, vp, i64],
        "mgf_batch_copy_worlds_where": [vp, vp, vp, vp, i64, vp],
    }
    assert set(want) == set(ENTRY_POINTS)
    for name, args in want.items():
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32 and list(fn.argtypes) == args, name
    for method in ("body_index", "gather_state", "set_velocities_dev", "set_forces_dev", "apply_impulses_dev", "body_contacts_dev", "copy_worlds_where"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    assert callable(mgf_amd.Context.synchronize)


def test_integration_md_has_the_rust_twins():
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for sig in ("pub fn mgf_ctx_synchronize(ctx: *mut mgf_ctx) -> mgf_status;",
                "pub fn mgf_batch_gather_state_dev(b: *mut mgf_batch, body_dev: *const i32, n: i64, x: *mut f32, q: *mut f32, v: *mut f32, "
                "omega: *mut f32, force: *mut f32, torque: *mut f32) -> mgf_status;",
                "pub fn mgf_batch_set_many_dev(b: *mut mgf_batch, body_dev: *const i32, n: i64, linear: *const f32, angular: *const f32) -> mgf_status;",
                "pub fn mgf_batch_set_forces_dev(b: *mut mgf_batch, body_dev: *const i32, n: i64, force: *const f32, torque: *const f32) -> mgf_status;",
                "pub fn mgf_batch_apply_impulses_dev(b: *mut mgf_batch, body_dev: *const i32, n: i64, linear: *const f32, angular: *const f32) -> mgf_status;",
                "pub fn mgf_batch_read_body_contacts_dev(b: *mut mgf_batch, world: i64, out_dev: *mut mgf_body_contacts, cap: i64) -> mgf_status;",
                "pub fn mgf_batch_copy_worlds_where(dst: *mut mgf_batch, dst_world: *const i32, src: *const mgf_batch, src_world: *const i32, "
                "n: i64, mask_dev: *const i32) -> mgf_status;"):
        assert sig in flat, sig


def test_what_needs_no_device_is_refused_before_the_handle_is_dereferenced():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced, a "device" address that is never looked up
    dev = C.c_void_p(4096)
    n = 4
    world = np.zeros(n, np.int32)
    calls = {
        "gather": lambda h, c=n: lib.mgf_batch_gather_state_dev(h, dev, c, dev, dev, dev, dev, dev, dev),
        "set": lambda h, c=n: lib.mgf_batch_set_many_dev(h, dev, c, dev, dev),
        "forces": lambda h, c=n: lib.mgf_batch_set_forces_dev(h, dev, c, dev, dev),
        "impulses": lambda h, c=n: lib.mgf_batch_apply_impulses_dev(h, dev, c, dev, dev),
    }
    for name, call in calls.items():
        assert call(None) == INV and "NULL" in err(), name
        assert call(fake, c=-1) == INV and "negative" in err(), name
        assert call(fake, c=-(1 << 40)) == INV and "negative" in err(), name
        assert call(fake, c=(1 << 31)) == INV and "too many" in err(), name
    # both arrays of mgf_batch_set_many_dev are required, whatever n
    for lin, ang in ((None, dev), (dev, None), (None, None)):
        assert lib.mgf_batch_set_many_dev(fake, dev, n, lin, ang) == INV and "NULL" in err()
        assert lib.mgf_batch_set_many_dev(fake, dev, 0, lin, ang) == INV and "NULL" in err()
    assert lib.mgf_batch_read_body_contacts_dev(None, 0, dev, n) == INV and "NULL" in err()
    assert lib.mgf_batch_read_body_contacts_dev(fake, 0, None, n) == INV and "NULL" in err()
    assert lib.mgf_batch_read_body_contacts_dev(fake, -2, dev, n) == INV and "world index" in err()
    # the masked copy: mgf_batch_copy_worlds' own refusals, in its words
    p = world.ctypes.data
    neg = world.copy()
    neg[2] = -1
    assert lib.mgf_batch_copy_worlds_where(None, p, fake, p, n, dev) == INV and "NULL" in err()
    assert lib.mgf_batch_copy_worlds_where(fake, p, None, p, n, dev) == INV and "NULL" in err()
    assert lib.mgf_batch_copy_worlds_where(fake, None, fake, p, n, dev) == INV and "NULL" in err()
    assert lib.mgf_batch_copy_worlds_where(fake, p, fake, None, n, dev) == INV and "NULL" in err()
    assert lib.mgf_batch_copy_worlds_where(fake, p, fake, p, -1, dev) == INV and "negative" in err()
    assert lib.mgf_batch_copy_worlds_where(fake, p, fake, p, 1 << 31, dev) == INV and "too many" in err()
    assert lib.mgf_batch_copy_worlds_where(fake, neg.ctypes.data, fake, p, n, dev) == INV and "world index" in err()
    assert lib.mgf_batch_copy_worlds_where(fake, p, fake, neg.ctypes.data, n, dev) == INV and "world index" in err()
    assert lib.mgf_ctx_synchronize(None) == INV and "NULL" in err()
    for name in (b"device_skipped", b"pair_table_uploads"):
        assert lib.mgf_batch_counter(None, name, C.byref(C.c_int64())) == INV


def test_every_device_pointer_is_looked_up_before_the_first_enqueue():
    """the order "check, then enqueue", read in the source: in every entry point of host_batch_dev.inc the last dev_span comes before
    the first thing that enqueues (a push of the mirror, a memset, a copy, a launch)"""
    src = read("mgf_amd", "csrc", "host_batch_dev.inc")
    bodies = re.split(r"\n(?=extern \"C\"|template <int MODE>\nstatic mgf_status batch_dev_set)", src)[1:]
    assert len(bodies) == 7, len(bodies)
    checked = 0
    for body in bodies:
        if "dev_span" not in body and "batch_dev_set<" in body:
            continue   # (the three setters: one line each into batch_dev_set)
        last_check = max(m.start() for m in re.finditer(r"dev_span\(|batch_dev_open\(", body))
        first_enqueue = min(m.start() for m in re.finditer(r"batch_push\(|batch_dev_begin\(|batch_copy_open\(|hipMemsetAsync|hipMemcpyAsync|<<<|prim_exclusive_scan_u32", body))
        assert last_check < first_enqueue, body[:120]
        checked += 1
    assert checked == 4
    opener = src[src.index("static mgf_status batch_dev_open"):src.index("static mgf_status batch_dev_begin")]
    assert "dev_span(" in opener and not re.search(r"batch_push|Async|<<<", opener)
    span = src[src.index("static mgf_status dev_span"):src.index("static mgf_status batch_dev_args")]
    assert "hipPointerGetAttributes" in span and "hipMemGetAddressRange" in span and "hipMemoryTypeDevice" in span and "hipMemoryTypeManaged" in span


def test_the_binding_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self):
            self._h, self.n_worlds = None, 1

        def __len__(self):
            return 4
    b = Handle()
    ok3, idx = torch.zeros((4, 3), dtype=torch.float32), torch.zeros(4, dtype=torch.int32)
    bad = {
        "dtype": torch.zeros((4, 3), dtype=torch.float64),
        "not contiguous": torch.zeros((3, 4), dtype=torch.float32).t(),
        "rows": torch.zeros((5, 3), dtype=torch.float32),
        "on cpu": ok3,
    }
    for what, t in bad.items():
        for call in (lambda: b.gather_state(None, x=t), lambda: b.gather_state(None, torque=t), lambda: b.set_velocities_dev(None, t, t),
                     lambda: b.set_forces_dev(None, None, t), lambda: b.apply_impulses_dev(None, t, None)):
            with pytest.raises(ValueError):
                call()
    for body in (torch.zeros(4, dtype=torch.int64), torch.zeros(8, dtype=torch.int32)[::2], idx):
        with pytest.raises(ValueError):
            b.set_forces_dev(body, None, None)
    with pytest.raises(ValueError):
        b.gather_state(idx, q=torch.zeros((4, 3), dtype=torch.float32))   # q has four columns
    with pytest.raises(ValueError):
        b.set_velocities_dev(None, None, ok3)
    with pytest.raises(ValueError):
        b.gather_state(1 << 20, x=None)                                     # a raw address needs n
    with pytest.raises(ValueError):
        b.gather_state(None, x=np.zeros((4, 3), np.float32))               # neither a tensor nor an address
    for mask in (None, torch.zeros(3, dtype=torch.float32), torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)):
        with pytest.raises(ValueError):
            b.copy_worlds_where([0, 0, 0], None, [0, 0, 0], mask)
    # what a tensor is checked for, and that a raw address passes as it is
    assert _capi._dev_arg(None, "float32", 3, 4, "x") is None and _capi._dev_arg(4096, "float32", 3, 4, "x") == 4096
    with pytest.raises(ValueError, match="on cpu"):
        _capi._dev_arg(ok3, "float32", 3, 4, "x")
    with pytest.raises(ValueError, match="dtype"):
        _capi._dev_arg(ok3, "int32", 3, 4, "x")


def test_the_new_kernels_use_no_scratch_spill_nothing_and_keep_their_lane_masks():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_dev_")
    assert set(rows) == NEW_KERNELS, rows
    bad = {k: v for k, v in rows.items() if (v[2], v[4], v[5]) != ("0", "0", "0")}
    assert not bad, bad
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_lane_masks.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 lane masks" in r.stdout, r.stdout


# ---- the GPU tests' inputs, without a GPU -------------------------------------------------------------------------------------------------
def test_the_scenes_and_records_are_what_the_gpu_tests_need():
    scs = DV.device_scenes()
    assert [len(sc["comps"]) for sc in scs] == [5, 1, 300]
    off = DV.offsets(scs)
    assert off.tolist() == [0, 5, 6, 306] and off[2] < DV.BLOCK < off[3]        # the world of 300 across two blocks of bodies
    flat = DV.records(scs)
    g3 = DV.triple_body(scs)
    assert len(flat) == DV.N_RECORDS > 2 * DV.BLOCK and len(set(flat.tolist())) == DV.N_DISTINCT
    at = np.flatnonzero(flat == g3)
    assert at.tolist() == list(DV.TRIPLE_AT) and len({int(k) // DV.BLOCK for k in at}) == 3 and g3 - off[2] > DV.BLOCK
    world, body = DV.world_body(scs, flat)
    assert DV.QUIET_WORLD not in world and set(world.tolist()) == {0, 2}
    assert np.array_equal(off[world] + body, flat)
    assert max(np.bincount(flat)) >= 3
    lin, _ = DV.impulse_rows(scs)
    x = [lin[k][0] for k in DV.TRIPLE_AT]
    assert (x[0] + x[1]) + x[2] != (x[0] + x[2]) + x[1] and all(v.dtype == np.float32 for v in x)   # the f32 sum depends on the order
    sub = DV.subset_with_repeats(scs)
    assert len(set(sub.tolist())) < len(sub) and {int(w) for w in DV.world_body(scs, sub)[0]} == {0, 1, 2} and np.any(np.diff(sub) < 0)
    assert sorted(DV.COPY_PAIRS.tolist()) == [0, 1, 2] and DV.COPY_PAIRS[1] == 2 and [list(m) for m in DV.MASKS] == [[1, 0, 1], [0, 0, 0], [1, 1, 1]]


def test_the_snapshot_of_the_masked_copy_outgrows_a_share_of_one_record_a_body():
    """measured: the world of 300 holds 457 constraints at tick 3 (cons_per_body = 1 gives it 300 records), the others 6 and 1 (16 each)"""
    scs = DV.device_scenes()
    counts = []
    for sc in scs:
        ow = oracle_world(sc)
        for _ in range(DV.TICKS):
            st = ow.step(float(sc["dt"]), sc["iters"])
        counts.append(int(st.n_constraints))
    assert counts[2] > 300 and 0 < counts[0] <= 16 and counts[1] <= 16, counts
