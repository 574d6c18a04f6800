"""The batch's observations (mgf_batch_read_body_contacts, mgf_batch_overlap_aabb_many) without a GPU: the header declares and defines
them, the library, the Python binding and INTEGRATION.md carry them, bad arguments are refused before the handle or a device is touched,
the kernels use no scratch memory and spill no register - and the inputs of the GPU test are not trivial, by the oracle alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_observe_cases as OC
from tests import batch_query_cases as BQ
from tests.util import ROOT, kernel_resources, oracle_world, read

ENTRY_POINTS = {
    "mgf_batch_read_body_contacts": r"mgf_status mgf_batch_read_body_contacts\(mgf_batch\* b, int64_t world, mgf_body_contacts\* out, int64_t cap\);",
    "mgf_batch_overlap_aabb_many": r"mgf_status mgf_batch_overlap_aabb_many\(mgf_batch\* b, const int32_t\* world, const mgf_aabb\* boxes, int64_t n,\s*"
                                   r"uint64_t\* out_offsets /\* n\+1 \*/, uint32_t\* out_bodies, int64_t cap, int64_t\* total\);",
}


def test_header_declares_and_defines_them():
    h = read("include", "mgf_hip.h")
    section = h[h.index("many small worlds"):]
    for name, sig in ENTRY_POINTS.items():
        assert re.search(r"MGF_API " + sig, section), name
    m = re.search(r"typedef struct mgf_body_contacts \{(.*?)\} mgf_body_contacts;", section, re.S)
    assert m, "mgf_body_contacts"
    fields = re.findall(r"^\s*(\w+) (\w+);", m.group(1), re.M)
    assert fields == [("int32_t", "n_contacts"), ("int32_t", "n_terrain"), ("mgf_vec3", "impulse"), ("float", "normal_impulse")], fields
    # the definition cites what it restates, says whose it is and what it leaves out
    for cite in ("solver.rs:203-252", "world.rs:243-291", "solver.rs:243-247", "bounds.rs:170-190", "collision.rs:22-29"):
        assert cite in section, cite
    for word in ("the reference has no such report", "Tangent impulses are not part of it", "mgf_constraint does not carry them",
                 "unchanged by mgf_batch_write_state", "out_offsets and *total are always filled"):
        assert word in section, word
    for text in (h, read("DESIGN.md")):
        assert "no box-overlap query" not in text
    readme = read("README.md")
    for name in ("read_body_contacts", "overlap_aabb_many"):
        assert name in readme[readme.index("mgf_batch_new"):], name


def test_library_and_binding_export_them():
    lib = mgf_amd.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _capi.SYMBOLS, name
    for method in ("body_contacts", "overlap_aabb", "overlap_boxes"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    assert mgf_amd.BODY_CONTACTS_DTYPE.itemsize == 24
    assert mgf_amd.BODY_CONTACTS_DTYPE.names == ("n_contacts", "n_terrain", "impulse", "normal_impulse")
    assert [mgf_amd.BODY_CONTACTS_DTYPE.fields[f][1] for f in mgf_amd.BODY_CONTACTS_DTYPE.names] == [0, 4, 8, 20]


def test_integration_md_has_the_rust_twins():
    text = read("INTEGRATION.md")
    assert "pub fn mgf_batch_read_body_contacts(b: *mut mgf_batch, world: i64, out: *mut mgf_body_contacts, cap: i64) -> mgf_status;" in text
    assert re.search(r"pub fn mgf_batch_overlap_aabb_many\(b: \*mut mgf_batch, world: \*const i32, boxes: \*const mgf_aabb, n: i64, out_offsets: \*mut u64,\s*"
                     r"out_bodies: \*mut u32, cap: i64, total: \*mut i64\) -> mgf_status;", text)
    assert re.search(r"#\[repr\(C\)\][^\n]*pub struct mgf_body_contacts \{ pub n_contacts: i32, pub n_terrain: i32, pub impulse: mgf_vec3, pub normal_impulse: f32 \}", text)
    wrapper = text[text.index("pub struct WorldBatch"):]
    for call in ("mgf_batch_read_body_contacts(self.raw", "mgf_batch_overlap_aabb_many(self.raw"):
        assert call in wrapper, call


def test_bad_arguments_are_refused_before_the_handle_or_a_device_is_touched():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    n = 4
    rec = np.zeros(n, _capi.BODY_CONTACTS_DTYPE)
    world = np.zeros(n, np.int32)
    boxes = np.zeros((n, 6), np.float32)
    off = np.zeros(n + 1, np.uint64)
    vals = np.zeros(16, np.uint32)
    total = C.c_int64()

    def overlap(h, w=world, q=boxes, count=n, o=off, v=vals, cap=16):
        return lib.mgf_batch_overlap_aabb_many(h, w.ctypes.data if w is not None else None, q.ctypes.data if q is not None else None, count,
                                               o.ctypes.data if o is not None else None, v.ctypes.data if v is not None else None, cap, C.byref(total))
    # a NULL handle
    assert lib.mgf_batch_read_body_contacts(None, 0, rec.ctypes.data, n) == INV and "NULL" in err()
    assert lib.mgf_batch_read_body_contacts(None, -1, rec.ctypes.data, n) == INV and "NULL" in err()
    assert overlap(None) == INV and "NULL" in err()
    # each refusal that needs no device, with a NULL handle and with one that is never dereferenced
    neg = world.copy()
    neg[2] = -1
    for h in (None, C.c_void_p(16)):
        assert lib.mgf_batch_read_body_contacts(h, 0, None, n) == INV and "NULL" in err()
        assert lib.mgf_batch_read_body_contacts(h, -1, None, n) == INV and "NULL" in err()
        for w in (-2, -(1 << 40)):   # (-1 is the whole batch)
            assert lib.mgf_batch_read_body_contacts(h, w, rec.ctypes.data, n) == INV and ("world index" in err() or h is None)
        for kw in (dict(w=None), dict(q=None), dict(o=None), dict(v=None)):
            assert overlap(h, **kw) == INV and "NULL" in err(), kw
        assert overlap(h, count=-1) == INV and ("negative" in err() or h is None)
        assert overlap(h, cap=-1) == INV and ("negative" in err() or h is None)
        assert overlap(h, w=neg) == INV and ("world index" in err() or h is None)
        assert overlap(h, count=(1 << 31), w=None, q=None) == INV   # (NULL arrays and too many: refused either way, nothing is read)


def test_the_kernels_use_no_scratch_and_spill_nothing():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_observe_")
    assert set(rows) == {"k_batch_observe_contacts", "k_batch_observe_overlap<false>", "k_batch_observe_overlap<true>"}, rows
    bad = {k: v for k, v in rows.items() if (v[2], v[4], v[5]) != ("0", "0", "0")}
    assert not bad, bad


# ---- the GPU test's inputs are not trivial: by the oracle alone ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def piles_at_30():
    scs = BQ.pile_scenes()
    out = []
    for sc in scs:
        ow = oracle_world(sc)
        for _ in range(30):
            ow.step(float(sc["dt"]), sc["iters"])
        out.append((sc, ow.constraints(), np.asarray(ow.state()["x"], np.float32)))
    return out


def test_the_piles_hold_every_kind_of_body(piles_at_30):
    """tick 30 of the 1024-sphere world: 1856 records, 1020 bodies touching, 64 records on terrain, 770 bodies occur as `b`, 4 in no record;
    the 512-sphere world has 952 records - and the fold of such a list has impulses in it"""
    cat = [OC.categories(cons, len(sc["comps"])) for sc, cons, _ in piles_at_30]
    assert cat[4] == (1856, 1020, 64, 770, 4), cat[4]
    assert cat[2][0] == 952, cat[2]
    assert cat[3] == (0, 0, 0, 0, 0) and cat[0][0] == 1
    sc, cons, _ = piles_at_30[4]
    f = OC.fold(cons, 1024)
    assert int(f["n_contacts"].sum()) == 2 * 1856 - 64 and int(f["n_terrain"].sum()) == 64
    assert np.sum(f["n_contacts"] == 0) == 4 and np.all(f["normal_impulse"][f["n_contacts"] == 0] == 0)
    assert np.sum(f["normal_impulse"] > 0) > 900 and np.sum(np.any(f["impulse"] != 0, axis=1)) > 900
    assert f["n_contacts"].max() >= 6


@pytest.mark.parametrize("hub_first", [True, False])
def test_the_hub_has_a_chain_longer_than_a_workgroup(hub_first):
    """300 records on the hub at ticks 1 and 2 - as `b` when it is body 0, as `a` when it is the last -, a normal_impulse of about 460 at
    tick 1, every other body in one record; and the 300-term f32 sums depend on the order: summed in reverse they differ"""
    sc, hub = OC.hub_scene(hub_first)
    ow = oracle_world(sc)
    shows = 0
    for tick in (1, 2):
        ow.step(float(sc["dt"]), sc["iters"])
        cons = ow.constraints()
        assert len(cons) == 300
        assert np.all((cons["b"] if hub_first else cons["a"]) == hub)
        f = OC.fold(cons, 301)
        assert f["n_contacts"][hub] == 300 and np.all(np.delete(f["n_contacts"], hub) == 1) and not np.any(f["n_terrain"])
        if tick == 1:
            assert 455.0 < f["normal_impulse"][hub] < 465.0, f["normal_impulse"][hub]
        back = OC.fold(cons[::-1], 301)     # the same records walked in the opposite order
        shows += int(back["normal_impulse"][hub] != f["normal_impulse"][hub]) + int(np.sum(back["impulse"][hub] != f["impulse"][hub]))
    assert shows >= 2, "the order of the sums does not show"


def test_the_capsule_scene_has_terrain_records_two_a_body():
    for sc in OC.capsule_scenes():
        ow = oracle_world(sc)
        seen = {}
        for tick in range(1, 41):
            ow.step(float(sc["dt"]), sc["iters"])
            if tick in (20, 40):
                cons = ow.constraints()
                f = OC.fold(cons, len(sc["comps"]))
                seen[tick] = (int(f["n_terrain"].max()), int(np.sum(cons["b"] >= 0)))
        assert seen[20][0] >= 2 and seen[40][0] >= 2 and seen[40][1] > 0, seen


def test_the_boxes_meet_none_one_and_many_bodies(piles_at_30):
    """the mixed boxes of the GPU test over the piles at tick 30: empty answers, single bodies and lists longer than a wave; and the special
    boxes: all 1024 bodies, none, the touching face (equality in f32), its neighbour, NaN, a negative half extent that still hits"""
    centres = [x for _, _, x in piles_at_30]
    world, boxes = OC.mixed_boxes(centres, BQ.COUNTS_T30)
    assert sorted(np.bincount(world, minlength=5).tolist()) == sorted(BQ.COUNTS_T30)
    lens = []
    for k, (sc, _, x) in enumerate(piles_at_30):
        comps = sc["comps"].copy()
        comps["p"] = x        # a sphere's collider is its position (construct, compound.rs:54-66)
        bx = OC.tight_boxes(comps)
        lens += [len(OC.overlaps(bx, q)) for q in boxes[world == k]]
    lens = np.array(lens)
    assert np.sum(lens == 0) > 10 and np.sum(lens == 1) > 10 and lens.max() > 64, (np.sum(lens == 0), np.sum(lens == 1), lens.max())
    comps = piles_at_30[4][0]["comps"].copy()
    comps["p"] = centres[4]
    bx = OC.tight_boxes(comps)
    sp = OC.special_boxes(bx)
    hits = [OC.overlaps(bx, q) for q in sp]
    assert len(hits[0]) == 1024 and len(hits[1]) == 0 and len(hits[4]) == 0
    assert 0 in hits[2] and 0 not in hits[3] and 0 in hits[5]
    assert np.float32(abs(np.float32(bx[0, 0] - sp[2, 0]))) == np.float32(bx[0, 3] + sp[2, 3]), "the touching box does not touch with equality"
