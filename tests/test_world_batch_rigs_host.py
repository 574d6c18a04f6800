"""What the three rigs of a batch - body-mounted ray sensors, depth cameras, box zones - share (host_batch_rig.inc, BatchRig in
host_batch.inc, bo_front in k_batch_observe.h), without a GPU and in one place: the plan of a rig is a partition into items of at most
256 records; the shared steps refuse without changing anything, upload in one copy and are written once; mgf_batch_add_bodies marks all
three rigs; and the batch's query kernels keep the figures DESIGN.md records, with no lane mask in the library."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import batch_query_device_cases as QD
from tests import batch_rig_cases as RC
from tests.util import RESOURCES, ROOT, kernel_resources, read


@pytest.mark.parametrize("case", range(len(RC.PLAN_IDS)), ids=RC.PLAN_IDS)
def test_the_plan_of_a_rig_is_a_partition_into_items_of_at_most_256(case):
    """mgf_batch_set_sensors and mgf_batch_set_zones sort the rig with the host's BatchQueryPlan: one stable counting sort.
    QD.plan_model is that plan with the ranks taken in array order - the host's order - so here the caller's relative order within a
    world is part of the claim"""
    name, whose, world, K, counts = RC.plan_cases()[case]
    n = len(world)
    items, order, skipped = QD.plan_model(world, K)
    assert skipped == 0 and sorted(order.tolist()) == list(range(n)), name
    seen = np.zeros(n, np.int64)
    for w, first, count in items:
        assert 1 <= count <= 256, (name, count)
        q = order[first:first + count]
        assert np.all(world[q] == w) and np.all(np.diff(q) > 0), name              # one world; the caller's relative order
        seen[q] += 1
    assert np.all(seen == 1), name
    assert np.all(np.diff(items[:, 0]) >= 0) and np.all(np.diff(items[:, 1]) > 0), name
    assert len(items) == sum((c + 255) // 256 for c in counts), name
    if whose == "sensors":
        assert np.any(np.diff(world) < 0), name                                    # shuffled world order
        assert np.bincount(world, minlength=K).tolist() == counts, name
        for w in range(K):                                                         # across a world's items too: ascending
            q = order[np.flatnonzero(world[order] == w)]
            assert np.all(np.diff(q) > 0), (name, w)
        if case == 0:
            assert items[:, 2].tolist() == [1, 256, 256, 1, 256, 256, 88]
    else:
        assert n == sum(counts)
        assert set(items[:, 0].tolist()) == {k for k, c in enumerate(counts) if c}, name    # a world without zones has no item
        if name == "257":
            assert items[:, 2].tolist() == [256, 1]
        if K > 1:
            assert np.any(np.diff(world) < 0) and items[:, 2].tolist() == [3, 256, 1, 65]
    # both set calls use that plan: the one plan step, reached from each
    plan = RC.plan_step()
    assert "const BatchQueryPlan plan(b->K, world.data(), n);" in plan and "plan.fill(world.data(), n, R.items.data(), R.order.data());" in plan
    assert "batch_rig_plan(b, b->sensors, s, n);" in read("mgf_amd", "csrc", RC.RIG_FILES["sensors"])
    assert "batch_rig_plan(b, b->zones, z, n);" in read("mgf_amd", "csrc", RC.RIG_FILES["zones"])


def test_the_shared_steps_are_written_once_and_refuse_without_changing_anything():
    rig = RC.rig_source()
    files = {k: read("mgf_amd", "csrc", f) for k, f in RC.RIG_FILES.items()}
    for fn in ("batch_rig_set_args", "batch_rig_ref_check", "batch_rig_plan", "batch_rig_upload", "batch_rig_up", "batch_rig_handle", "batch_rig_cap",
               "batch_rig_fits"):
        assert len(re.findall(r"^(?:template <class Rec>\n)?static \w+ " + fn + r"\(", rig, re.M)) == 1, fn
        for name, text in files.items():
            assert not re.search(r"^static \w+ " + fn + r"\(", text, re.M), (fn, name)
    # none of the three writes what the shared steps write: no copy of the plan, of the upload or of the four refusals is left
    for name, text in files.items():
        for gone in ("BatchQueryPlan plan(", "batch_rig_upload(", "names a body its world does not hold", '"batch is NULL"', '"cap is negative"',
                     '"buffer too small"'):
            assert gone not in text, (name, gone)
        assert text.count("batch_rig_set_args(b, ") == 1 and text.count("batch_rig_up(b, R, ") == 1, name
    # the set prologue: the handle and n, then the NULL records
    pro = RC.set_args_step()
    assert pro.index("batch_dev_args(b, n_in)") < pro.index('"NULL argument"') < pro.index("return MGF_OK;")
    # the record check refuses; it changes nothing (its messages: tests/test_world_batch_{sensors,cameras,zones}_host.py)
    check = RC.ref_check_step()
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(|b->\w+ =[^=]", check)
    # the plan step needs no device, and the stale flag is the last thing it sets
    plan = RC.plan_step()
    assert not re.search(r"<<<|Async|hipMalloc|\.ensure\(|h2d\(", plan)
    assert plan.index("R.recs.assign(recs, recs + n);") < plan.index("plan.fill(") < plan.index("R.stale = true;")
    # the upload: nothing while the copy is fresh; the bodies against the lengths again, with the rig's word; ONE copy; then fresh
    up = RC.up_step()
    assert (up.index("if (!R.stale) return MGF_OK;") < up.index('"internal error: a %s names a body its world does not hold", what')
            < up.index("batch_rig_upload(b, R.dev, sec, n_sec, R.off)") < up.index("R.stale = false;"))
    assert up.count("batch_rig_upload(") == 1 and "h2d(" not in up and "!(or_world && r.body < 0) && (uint32_t)r.body >= b->h_n[(size_t)r.world]" in up
    upload = RC.upload_step()
    assert upload.count("h2d(") == 1 and upload.count(".ensure(") == 1 and "<<<" not in upload          # the steady state uploads nothing; ONE copy
    # the layouts are arguments of that step: the sensors' four sections, the cameras' two, the zones' three with a body of -1 let through
    assert 'batch_rig_up(b, R, "sensor", 4)' in files["sensors"] and 'batch_rig_up(b, R, "camera", 2)' in files["cameras"]
    assert 'batch_rig_up(b, R, "zone", 3, true)' in files["zones"]
    # one type holds the three rigs, and mgf_batch_add_bodies marks all of them through one step
    host = read("mgf_amd", "csrc", "host_batch.inc")
    for member in ("BatchRig<mgf_batch_sensor> sensors;", "BatchRig<mgf_batch_camera> cameras;", "BatchRig<mgf_batch_zone> zones;"):
        assert host.count(member) == 1, member
    assert not re.search(r"\b[scz]_(rig|items|tiles|order|stale|dev|o_rig|o_order|o_world)\b", host + rig + "".join(files.values()))
    stale = RC.stale_step()
    assert "b->sensors.stale = true;" in stale and "b->cameras.stale = true;" in stale and "b->zones.stale = true;" in stale
    add = host[host.index('extern "C" mgf_status mgf_batch_add_bodies('):]
    assert "batch_rigs_stale(b);" in add[:add.index("\n}\n")]
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_query_dev.inc"') < hip.index('#include "host_batch_rig.inc"') < hip.index('#include "host_batch_sensor.inc"')


def test_the_overlap_front_is_written_once():
    o, z = read("mgf_amd", "csrc", "k_batch_observe.h"), read("mgf_amd", "csrc", "k_batch_zone.h")
    near, part, q = read("mgf_amd", "csrc", "k_batch_nearest.h"), read("mgf_amd", "csrc", "k_batch_part_query.h"), read("mgf_amd", "csrc", "k_batch_query.h")
    assert o.count("uint32_t bo_front(") == 1
    for other in (z, near, part):
        assert "bo_front(" not in other.replace("bo_front<", "")
    assert '#include "k_batch_observe.h"' in z
    half = o[o.index("struct BatchOverlapArgs"):]                        # (the overlap half of the file: behind k_batch_observe_contacts)
    for text in ("__ballot(", "__syncthreads()", "min(W.shift(), 6u)"):
        assert half.count(text) == 1, text
        for other in (z, near) if text == "__syncthreads()" else (z, near, part):
            assert text not in other[other.index("#pragma once"):], text
    # (the part rows' one barrier is the end of their ray and sweep staging; no box kernel runs it)
    code = part[part.index("#pragma once"):]
    assert code.count("__syncthreads()") == 1 and code.index("void pq_stage(") < code.index("__syncthreads()") < code.index("// the body-level rejects")
    # across the batch's headers: the box front's split once; its ballot the only one of a box query (the cameras' tile compaction
    # and the parts' tick have their own, which are no box front)
    assert sum(read("mgf_amd", "csrc", f).count("min(W.shift(), 6u)") for f in _batch_headers()) == 1
    assert {f for f in _batch_headers() if "__ballot(" in read("mgf_amd", "csrc", f)} == {"k_batch_observe.h", "k_batch_camera.h", "k_batch_parts.h"}
    # a body's box comes from the bodies' policy; the plain one is the collider row's tight bounds, written once
    assert half.count("bodies.box((size_t)g0 + i)") == 1 and "comp_bounds(" not in half
    plain = q[q.index("struct PlainBodies {"):q.index("void bq_ray_front(")]
    assert plain.count("comp_bounds(to_comp(A.col0[g], A.col1[g]))") == 1
    assert sum(read("mgf_amd", "csrc", f).count("comp_bounds(to_comp(A.col0[") for f in _batch_headers()) == 1
    for other in (z, near):
        assert "comp_bounds(to_comp(" not in other[other.index("#pragma once"):]
    # the overlap kernels have no ignored body, the zones have; the fixed layout has no order array
    assert o.count("bo_front<false, false>(") == 1 and "(!IGNORE || (int32_t)i != ign)" in o
    assert ("SRC == kItemFixed ? bo_front<true, true>(A, bodies, W, s_dyn, z, fixed, store) : bo_front<false, true>(A, bodies, W, s_dyn, z, mounted, store)"
            in z)
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert "bo_front" in kernels[kernels.index("k_batch_observe_contacts / _overlap<FILL>"):kernels.index("k_batch_zone_first<SRC>")]


def _batch_headers():
    return sorted(f for f in os.listdir(os.path.join(ROOT, "mgf_amd", "csrc")) if f.startswith("k_batch_") and f.endswith(".h"))


def test_every_query_front_is_written_once():
    """The guard that the fronts of the batch's query kernels stay written once: the defining line of each occurs once across
    mgf_amd/csrc/k_batch_*.h, and no header asks that a change be made twice."""
    text = {f: read("mgf_amd", "csrc", f) for f in _batch_headers()}
    assert len(text) >= 17, sorted(text)
    once = {
        "the ray front": "__device__ __forceinline__ void bq_ray_front(",
        "the sweep front": "__device__ __forceinline__ void bq_sweep_front(",
        "the box front": "__device__ __forceinline__ uint32_t bo_front(",
        "the overlap kernels' body": "__device__ __forceinline__ void bo_overlap(",
        "the zone-first kernels' body": "__device__ __forceinline__ void bz_first(",
        "the nearest kernels' body": "__device__ __forceinline__ void bn_nearest(",
        "the zones' fixed loader": "__device__ __forceinline__ BatchBox bz_fixed(",
        "the zones' mounted loader": "__device__ __forceinline__ BatchBox bz_mounted(",
        "the zones' box store": "__device__ __forceinline__ void bz_box_out(",
        "the sensors' loader and store": "__device__ __forceinline__ void bs_rays(",
        "the feelers' loader and store": "__device__ __forceinline__ void bf_casts(",
    }
    where = {"bq_ray_front(": "k_batch_query.h", "bq_sweep_front(": "k_batch_query.h", "bo_front(": "k_batch_observe.h", "bo_overlap(": "k_batch_observe.h",
             "bz_first(": "k_batch_zone.h", "bn_nearest(": "k_batch_nearest.h", "bz_fixed(": "k_batch_zone.h", "bz_mounted(": "k_batch_zone.h",
             "bz_box_out(": "k_batch_zone.h", "bs_rays(": "k_batch_sensor.h", "bf_casts(": "k_batch_feeler.h"}
    for what, line in once.items():
        assert sum(t.count(line) for t in text.values()) == 1, what
        fn = line.split()[-1]
        assert line in text[where[fn]], what
        assert len(re.findall(r"^[^/\n]*\b(?:void|uint32_t|BatchBox) " + re.escape(fn), "".join(text.values()), re.M)) == 1, what     # however it is spelt
    # the loaders' and stores' own lines: once each
    for line in ("const SensorIn s = A.rig[qi];", "const FeelerIn f = A.rig[qi];", "const ZoneIn s = A.rig[qi];", "A.casts[qi] = m;",
                 "float* o = A.parts + 7 * (size_t)qi;", "float* bo = boxes_out + 6 * (size_t)qi;", "for (uint32_t r0 = 0; r0 < k; r0 += 4u)",
                 "if (hit && rank < k) record()[1u + rank] = (int32_t)i;", "if (FILL && hit) A.out[base + rank] = i;",
                 "q_ray_store(A.out + 7 * (size_t)qi, best);", "q_sweep_store(A.out + 13 * (size_t)qi, best);"):
        assert sum(t.count(line) for t in text.values()) == 1, line
    for f, t in text.items():
        assert "KEEP IN STEP" not in t, f
    for f in ("k_batch_query.h", "k_batch_query_dev.h", "k_batch_sensor.h", "k_batch_feeler.h", "k_batch_observe.h", "k_batch_zone.h", "k_batch_nearest.h",
              "k_batch_part_query.h"):
        assert "restated" not in text[f] and "a second time" not in text[f], f
    # both policies of the bodies are named where the fronts stand
    q = text["k_batch_query.h"]
    assert "struct PlainBodies {" in q and "PartBodies (k_batch_part_query.h)" in q and "struct PartBodies {" in text["k_batch_part_query.h"]


def test_the_query_kernels_keep_their_figures_and_the_library_holds_no_lane_mask():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    old = kernel_resources("k_batch_query_")
    assert set(old) == set(RESOURCES), sorted(old)
    for name, want in RESOURCES.items():
        assert old[name] == want, (name, old[name], want)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_lane_masks.py")], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 lane masks" in r.stdout, r.stdout[-400:]
