"""The batch's bodies of up to four components without a GPU: the header, the library, the binding and INTEGRATION.md declare
mgf_batch_add_compound_bodies, its bad arguments are refused before the batch or a device is looked at, the part-aware tick's kernels are
built - without scratch memory or spills - and DESIGN.md names them with their compiler figures."""
import ctypes as C
import re

import numpy as np

import mgf_amd
from mgf_amd import _capi, scenes
from tests.util import kernel_resources, read

NAME = "mgf_batch_add_compound_bodies"
SIG = (r"MGF_API mgf_status mgf_batch_add_compound_bodies\(mgf_batch\* b, int64_t world, const mgf_component\* comps, const float\* comp_mass,\s*"
       r"const int64_t\* offsets /\* n \+ 1 \*/, int64_t n, const float\* restitution,\s*const float\* friction, const mgf_vec3\* world_force, uint64_t\* first_id\);")
TICK_KERNELS = ("k_batch_parts_front", "k_batch_parts_faces", "k_batch_parts_obst", "k_batch_parts_pairs", "k_batch_parts_pack")


def test_header_library_binding_and_integration_md_declare_the_entry_point():
    h = read("include", "mgf_hip.h")
    assert re.search(SIG, h)
    batch = h[h.index("many small worlds"):]
    assert "several components" in batch and "the batch takes four, the lone world 32" in batch
    for refused in ("mgf_batch_raycast_many(_dev)", "_sweep_many(_dev)", "_overlap_aabb_many", "_overlap_first_dev", "_cast_sensors(_dev)", "_cast_cameras(_dev)",
                    "_read_zones(_dev)"):
        assert refused in batch, refused
    assert "bodies of one component (spheres and capsules)" not in h
    lib = mgf_amd.load_library()
    assert hasattr(lib, NAME) and NAME in _capi.SYMBOLS
    assert hasattr(mgf_amd.WorldBatch, "add_compound_bodies")
    text = read("INTEGRATION.md")
    assert re.search(r"pub fn mgf_batch_add_compound_bodies\(b: \*mut mgf_batch, world: i64, comps: \*const mgf_component, comp_mass: \*const f32, offsets: \*const i64,", text)
    assert "pub fn add_compound_bodies(&mut self, world: usize" in text


def _comps(tags):
    c = np.zeros(len(tags), scenes.COMPONENT_DTYPE)
    c["tag"] = tags
    c["p"][:, 0] = np.arange(len(tags))
    c["d"][:, 1] = 1.0
    c["r"] = 0.4
    return c


def test_bad_arguments_are_refused_before_the_batch_or_a_device_is_touched():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID
    ones = np.ones(4096, np.float32)
    force = np.zeros((2048, 3), np.float32)
    first = C.c_uint64(77)

    def err():
        return lib.mgf_last_error().decode()

    def add(h, world, comps, offsets, n=None, first_id=first, off_null=False):
        off = np.ascontiguousarray(offsets, np.int64)
        return lib.mgf_batch_add_compound_bodies(h, world, None if comps is None else comps.ctypes.data, ones.ctypes.data, None if off_null else off.ctypes.data,
                                                 len(off) - 1 if n is None else n, ones.ctypes.data, ones.ctypes.data, force.ctypes.data,
                                                 None if first_id is None else C.byref(first_id))
    four = _comps([0, 1, 1, 0])
    assert add(None, 0, four, [0, 4]) == INV and "NULL" in err()
    fake = C.c_void_p(16)  # never dereferenced: every check below comes before the batch or a device is looked at
    assert add(fake, 0, None, [0, 4]) == INV and "NULL" in err()
    assert add(fake, 0, four, [0, 4], off_null=True) == INV and "NULL" in err()
    assert add(fake, 0, four, [0, 4], first_id=None) == INV and "NULL" in err()
    assert add(fake, 0, four, [0, 4], n=-1) == INV and "negative" in err()
    for world in (-1, -(1 << 40)):
        assert add(fake, world, four, [0, 4]) == INV and "world index" in err()
    assert add(fake, 0, four, [1, 4]) == INV and "offsets[0]" in err()
    five = _comps([0, 1, 1, 0, 0])
    for offsets in ([0, 5], [0, 0], [0, 2, 2, 4], [0, 4, 3]):  # five components, none, none in the middle, a negative count
        comps = five if offsets[-1] == 5 else four
        assert add(fake, 0, comps, offsets) == INV, offsets
        assert "the batch takes four, the lone world 32" in err(), offsets
    assert add(fake, 0, _comps([0, 2]), [0, 2]) == INV and "tag" in err()
    assert add(fake, 0, _comps([0, -1, 1]), [0, 1, 3]) == INV and "tag" in err()
    many = np.arange(1026, dtype=np.int64)  # 1025 bodies of one component each: more than any world holds
    assert add(fake, 0, _comps([0] * 1025), many) == INV and "MGF_BATCH_MAX_BODIES" in err()
    assert first.value == 77  # (nothing was written)


def test_the_part_aware_tick_kernels_are_built_without_scratch_or_spills():
    rows = kernel_resources("k_batch_")
    for name in TICK_KERNELS + ("k_batch_parts_copy",):
        assert name in rows, f"{name} is not in the library"
        vgpr, sgpr, scratch, lds, sspill, vspill = rows[name]
        assert (scratch, sspill, vspill) == ("0", "0", "0"), (name, rows[name])
    assert not any("k_batch_query_" in n and "parts" in n for n in rows)
    # the tick of a batch without such bodies is still there under its plain names
    for name in ("k_batch_front", "k_batch_faces", "k_batch_pairs", "k_batch_pack", "k_batch_setup", "k_batch_solve"):
        assert name in rows, name


def test_design_md_names_the_kernels_with_their_figures():
    text = read("DESIGN.md")
    at = text.index("### Bodies of up to four components")
    section = text[at:]
    rows = kernel_resources("k_batch_parts_")
    for name in TICK_KERNELS:
        vgpr, sgpr, scratch, lds, sspill, vspill = rows[name]
        m = re.search(r"\| `" + name + r"` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|", section)
        assert m, f"DESIGN.md has no row of figures for {name}"
        assert m.groups() == (vgpr, sgpr, scratch, lds, str(int(sspill) + int(vspill))), (name, m.groups(), rows[name])
    assert "seven launches" in section and "several components" in section
    assert "four" in read("README.md")[read("README.md").index("mgf_batch_add_compound_bodies"):][:2000]
