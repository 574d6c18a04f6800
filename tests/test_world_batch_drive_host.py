"""Driving a batch (mgf_batch_get_many, _set_many, _set_forces, _apply_impulses, _copy_worlds) without a GPU: the header declares the
calls, the library, the Python binding and INTEGRATION.md carry them, NULL and negative arguments are refused before the handle is
dereferenced, the kernels use no scratch memory, spill nothing and pass the lane-mask check - and the conditions that keep the GPU
tests from passing vacuously hold, by the oracle alone."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_drive_cases as DC
from tests.util import ROOT, kernel_resources, oracle_world, read

REC = r"mgf_batch\* b, const int32_t\* world, const int32_t\* body, int64_t n,\s*"
ENTRY_POINTS = {
    "mgf_batch_get_many": r"mgf_status mgf_batch_get_many\(" + REC + r"mgf_velocity\* vel, mgf_rigid_body_info\* info, mgf_vec3\* force, mgf_vec3\* torque\);",
    "mgf_batch_set_many": r"mgf_status mgf_batch_set_many\(" + REC + r"const mgf_velocity\* vel\);",
    "mgf_batch_set_forces": r"mgf_status mgf_batch_set_forces\(" + REC + r"const mgf_vec3\* force, const mgf_vec3\* torque\);",
    "mgf_batch_apply_impulses": r"mgf_status mgf_batch_apply_impulses\(" + REC + r"const mgf_vec3\* linear, const mgf_vec3\* angular\);",
    "mgf_batch_copy_worlds": r"mgf_status mgf_batch_copy_worlds\(mgf_batch\* dst, const int32_t\* dst_world, const mgf_batch\* src, const int32_t\* src_world, int64_t n\);",
}


def test_header_declares_the_calls_and_says_what_they_leave_out():
    h = read("include", "mgf_hip.h")
    section = h[h.index("many small worlds"):]
    for name, sig in ENTRY_POINTS.items():
        assert re.search(r"MGF_API " + sig, section), name
    for cite in ("physics.rs:272-304", "physics.rs:306-314", "physics.rs:146-147", "physics.rs:236, 240", "physics.rs:207", "physics.rs:212-214",
                 "solver.rs:243-247", "physics.rs:140"):
        assert cite in section, cite
    for word in ("drive_launches", "OUT OF SCOPE", "no force setter", "impulses at a point", "a whole-batch clone", "copies between contexts",
                 "no fused multiply-add", "a body named twice keeps the last", "the terrain assignment"):
        assert word in section, word
    design = read("DESIGN.md")
    assert "Driving a batch" in design and "stable sort" in design[design.index("Driving a batch"):]
    readme = read("README.md")
    for name in ("get_many", "set_forces", "apply_impulses", "copy_worlds"):
        assert name in readme[readme.index("mgf_batch_new"):], name
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert "k_batch_drive.h" in kernels and "k_batch_drive_get" in kernels


def test_library_and_binding_export_them():
    lib = mgf_amd.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _capi.SYMBOLS, name
    for method in ("get", "set_velocities", "set_forces", "apply_impulses", "copy_worlds"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    dt = mgf_amd.BODY_GET_DTYPE
    assert dt.names == ("linear", "angular", "x", "restitution", "friction", "inv_mass", "inv_moment", "force", "torque")
    assert dt.itemsize == 4 * (6 + 15 + 6)


def test_integration_md_has_the_rust_twins():
    text = read("INTEGRATION.md")
    flat = re.sub(r"\s+", " ", text)
    for sig in ("pub fn mgf_batch_get_many(b: *mut mgf_batch, world: *const i32, body: *const i32, n: i64, vel: *mut mgf_velocity, "
                "info: *mut mgf_rigid_body_info, force: *mut mgf_vec3, torque: *mut mgf_vec3) -> mgf_status;",
                "pub fn mgf_batch_set_many(b: *mut mgf_batch, world: *const i32, body: *const i32, n: i64, vel: *const mgf_velocity) -> mgf_status;",
                "pub fn mgf_batch_set_forces(b: *mut mgf_batch, world: *const i32, body: *const i32, n: i64, force: *const mgf_vec3, "
                "torque: *const mgf_vec3) -> mgf_status;",
                "pub fn mgf_batch_apply_impulses(b: *mut mgf_batch, world: *const i32, body: *const i32, n: i64, linear: *const mgf_vec3, "
                "angular: *const mgf_vec3) -> mgf_status;",
                "pub fn mgf_batch_copy_worlds(dst: *mut mgf_batch, dst_world: *const i32, src: *const mgf_batch, src_world: *const i32, "
                "n: i64) -> mgf_status;"):
        assert sig in flat, sig
    wrapper = text[text.index("pub struct WorldBatch"):]
    for name in ENTRY_POINTS:
        assert name + "(self.raw" in wrapper, name


def test_null_and_negative_arguments_are_refused_before_the_handle_is_dereferenced():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    n = 4
    world, body = np.zeros(n, np.int32), np.zeros(n, np.int32)
    vel, info = np.zeros((n, 6), np.float32), np.zeros((n, 15), np.float32)
    f3, t3 = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)

    def p(a):
        return None if a is None else a.ctypes.data
    calls = {
        "get": lambda h, w=world, b=body, c=n: lib.mgf_batch_get_many(h, p(w), p(b), c, p(vel), p(info), p(f3), p(t3)),
        "set": lambda h, w=world, b=body, c=n: lib.mgf_batch_set_many(h, p(w), p(b), c, p(vel)),
        "forces": lambda h, w=world, b=body, c=n: lib.mgf_batch_set_forces(h, p(w), p(b), c, p(f3), p(t3)),
        "impulses": lambda h, w=world, b=body, c=n: lib.mgf_batch_apply_impulses(h, p(w), p(b), c, p(f3), p(t3)),
        "copy": lambda h, w=world, b=body, c=n: lib.mgf_batch_copy_worlds(h, p(w), h, p(b), c),
    }
    neg = world.copy()
    neg[2] = -1
    for name, call in calls.items():
        assert call(None) == INV and "NULL" in err(), name
        fake = C.c_void_p(16)   # a handle that is never dereferenced: every check below comes before the batch or a device is looked at
        assert call(fake, w=None) == INV and "NULL" in err(), name
        assert call(fake, b=None) == INV and "NULL" in err(), name
        assert call(fake, c=-1) == INV and "negative" in err(), name
        assert call(fake, c=-(1 << 40)) == INV and "negative" in err(), name
        assert call(fake, c=(1 << 31)) == INV and "too many" in err(), name
        assert call(fake, w=neg) == INV and "world index" in err(), name
        assert call(fake, b=neg) == INV and ("body index" in err() or (name == "copy" and "world index" in err())), name
    assert lib.mgf_batch_set_many(C.c_void_p(16), p(world), p(body), n, None) == INV and "NULL" in err()
    assert lib.mgf_batch_set_many(C.c_void_p(16), p(world), p(body), 0, None) == INV and "NULL" in err()
    assert lib.mgf_batch_copy_worlds(C.c_void_p(16), p(world), None, p(body), n) == INV and "NULL" in err()
    assert lib.mgf_batch_counter(None, b"drive_launches", C.byref(C.c_int64())) == INV


def test_the_kernels_use_no_scratch_spill_nothing_and_keep_their_lane_masks():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_drive_")
    assert set(rows) == {"k_batch_drive_get", "k_batch_drive_set<0>", "k_batch_drive_set<1>", "k_batch_drive_set<2>", "k_batch_drive_copy"}, rows
    bad = {k: v for k, v in rows.items() if (v[2], v[4], v[5]) != ("0", "0", "0")}
    assert not bad, bad
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_lane_masks.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 lane masks" in r.stdout, r.stdout


# ---- the GPU tests' inputs are not trivial: by the oracle alone ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forced_run():
    scs = [DC.with_force(sc, DC.WORLD_FORCES[k]) for k, sc in enumerate(DC.drive_scenes())]
    return scs, DC.run_oracles(scs, DC.SWITCH_TICK)


def test_every_world_of_test_1_collides(forced_run):
    """measured: the piles hold 79-87 constraints at tick 1 and 100-117 at most, the capsule field 37 at most (tick 40: 36)"""
    scs, (_, hist, _) = forced_run
    assert [len(sc["comps"]) for sc in scs] == [64] * 5 + [48]
    assert len({tuple(f) for f in DC.WORLD_FORCES.tolist()}) == len(scs)
    assert all(np.all(sc["mass"] == 1.0) for sc in scs)   # force = world_force * mass is exact
    most = [max(c[0] for c, _ in h) for h in hist]
    assert all(m >= 30 for m in most), most
    assert all(hist[k][0][0][0] >= 70 for k in range(5)), [h[0][0] for h in hist]
    world, body = DC.all_bodies(scs, 3)
    assert len(world) == 5 * 64 + 48 and np.any(np.diff(world) < 0)   # one call, records of the worlds interleaved


def test_after_the_switch_every_world_has_terrain_and_pair_constraints(forced_run):
    """measured over the 20 ticks: piles (97, 16) .. (112, 25), capsule field (29, 25) .. (48, 34) as (all, terrain)"""
    scs, (ows, _, _) = forced_run
    world, body = DC.switched(scs)
    assert 100 < len(world) < 140 and set(np.unique(world).tolist()) == set(range(6)) and np.all(body % 3 == 0)
    for k, (sc, ow) in enumerate(zip(scs, ows)):
        fw = oracle_world(DC.with_force(sc, DC.switched_force(sc, k)))
        fw.set_state(**ow.state())
        both = False
        for _ in range(DC.SWITCH_RUN):
            st = fw.step(float(sc["dt"]), sc["iters"])
            both = both or (st.n_terrain_constraints > 0 and st.n_constraints > st.n_terrain_constraints)
        assert both, k


def test_the_fan_out_source_has_constraints_at_tick_20():
    sc = DC.fan_scene()
    assert len(sc["comps"]) == 12
    ow = oracle_world(sc)
    for _ in range(DC.FAN_TICKS):
        st = ow.step(float(sc["dt"]), sc["iters"])
    assert st.n_constraints > 0 and len(ow.constraints()) == st.n_constraints
    body, lin, ang = DC.fan_impulses()
    assert len(body) == DC.FAN_K and len(set(map(tuple, lin.tolist()))) == DC.FAN_K


def test_the_inputs_of_the_other_tests():
    scs = DC.drive_scenes()
    world, body, lin, ang = DC.velocity_commands(scs)
    pairs = list(zip(world.tolist(), body.tolist()))
    assert len(pairs) == 150 and len(set(pairs)) < 125          # bodies named again ...
    last = {}
    for k, pr in enumerate(pairs):
        last[pr] = k
    assert any(not np.array_equal(lin[k], lin[last[pr]]) for k, pr in enumerate(pairs))   # ... with another velocity
    world, body, lin, ang = DC.impulse_records(scs)
    at = [k for k in range(len(world)) if (world[k], body[k]) == (2, 5)]
    assert len(at) >= 3 and len(set(world[at[0]:at[-1] + 1].tolist())) > 1   # records of other worlds between the three
    # the definition's arithmetic: three records on one body are three sequential updates
    before = np.zeros(len(world), mgf_amd.BODY_GET_DTYPE)
    before["inv_mass"] = 0.5
    before["inv_moment"] = np.float32([2, 0, 0, 0, 3, 0, 0, 0, 4])
    v, w = DC.impulses_expected(before, world, body, lin, ang)
    want = np.float32([0, 0, 0])
    for k in at:
        want = want + lin[k] * np.float32(0.5)
    assert np.array_equal(v[at[0]], want) and np.array_equal(v[at[0]], v[at[-1]])
    # torque: spheres and capsules, half the bodies, three phases
    for k, sc in enumerate(DC.torque_scenes()):
        assert len(sc["comps"]) == 8 and sc["terrain"] is None and set(sc["comps"]["tag"].tolist()) == {0, 1}
        sched = DC.torque_schedule(k)
        assert sorted(sched) == [0, 10, 20] and len(sched[0][0]) == 4 and np.any(sc["comps"]["tag"][sched[0][0]] == 1)
        assert np.any(sched[0][1] != sched[10][1]) and not np.any(sched[20][1])
        assert np.any(sc["omega0"] != 0)
