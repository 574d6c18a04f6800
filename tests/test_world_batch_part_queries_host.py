"""The part-aware queries of a batch (mgf_batch_set_option "part_queries"; k_batch_part_query.h, host_batch_part_query.inc), read in the
source and in the built library without a device: the header names the option and its scope, the new kernels exist under k_batch_pq_
with no scratch and no spills, DESIGN.md carries their figures, no new file puts a kernel under a prefix whose kernel set other tests
pin, the host chooses the part-aware body pass behind every in-scope call and never for the cameras, the Python wrapper takes the
option."""
import inspect
import re

from tests import batch_part_query_cases as QC
from tests.util import kernel_resources, read


def test_header_names_the_option_and_the_scope():
    h = read("include", "mgf_hip.h")
    assert '"part_queries"' in h and "PART QUERIES" in h and "OUT OF SCOPE: mgf_batch_cast_cameras(_dev) stay refused" in h
    para = h[h.index("PART QUERIES:"):h.index("#define MGF_BATCH_MAX_BODIES")]
    for word in ("default 0", "(t, kind, index, part)", "radius-0 sphere at the centre of mass", "mgf_batch_write_state and mgf_batch_set_many move no part",
                 "_overlap_nearest_dev", "_read_zones_nearest(_dev)", "_cast_feelers(_dev)", "_cast_sensors(_dev)", "bit for bit"):
        assert word in para, word
    # the Limits paragraph keeps its sentences (tests/test_world_batch_parts_host.py reads them)
    assert "they do not see\n * parts yet" in h and "the batch takes four, the lone world 32" in read("mgf_amd", "csrc", "host_batch.inc")
    opt = h[h.index("/* Options (test knobs)"):h.index("MGF_API mgf_status mgf_batch_set_option")]
    assert '"part_queries" [0] = 0 | 1' in opt and "MGF_ERR_INVALID" in opt


def test_the_option_and_the_refusal_in_the_host_source():
    host = read("mgf_amd", "csrc", "host_batch.inc")
    opt = host[host.index('if (!strcmp(key, "part_queries"))'):host.index('return fail(MGF_ERR_INVALID, "unknown batch option")')]
    assert "value != 0 && value != 1" in opt and "b->part_queries = value == 1;" in opt and "bool part_queries = false;" in host
    gate = host[host.index("static mgf_status batch_single_parts("):host.index("// Bodies of 1..4 components for one world")]
    assert "bool part_aware = true" in gate and "if (!b->parts || (part_aware && b->part_queries)) return MGF_OK;" in gate
    assert "which this call does not see yet" in gate                       # the refusal's text is unchanged
    cam = read("mgf_amd", "csrc", "host_batch_camera.inc")
    assert cam.count("batch_single_parts(b,") == 2 and cam.count(", false))") == 2 and "batch_part_queries" not in cam and "batch_pq_" not in cam
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch.inc"') < hip.index('#include "host_batch_part_query.inc"') < hip.index('#include "host_batch_query.inc"')
    assert '#include "k_batch_part_query.h"' in read("mgf_amd", "csrc", "kernels.h")


def test_every_in_scope_call_chooses_the_part_aware_body_pass():
    new = read("mgf_amd", "csrc", "host_batch_part_query.inc")
    assert "static bool batch_part_queries(const mgf_batch* b) { return b->parts && b->part_queries; }" in new
    assert "36u * batch_nmax(b) + 16u * kBatchQueryRed" in new and "hipFuncSetAttribute" not in new
    assert "hipStreamSynchronize" not in new and "hipMemcpy" not in new and "q_launches" not in new      # a helper is the one launch it stands for
    assert new.count("<<<") == 7 and len(re.findall(r"k_batch_pq_\w+(?:<\w+>)?<<<", new)) == 7
    sites = {"host_batch_query.inc": 2, "host_batch_query_dev.inc": 2, "host_batch_sensor.inc": 1, "host_batch_feeler.inc": 1, "host_batch_zone.inc": 2,
             "host_batch_nearest.inc": 2, "host_batch_observe.inc": 2}
    for f, n in sites.items():
        src = read("mgf_amd", "csrc", f)
        assert "batch_part_queries(b)" in src and len(re.findall(r"MGF_TRY\(batch_pq_\w+(?:<\w+>)?\(", src)) == n, f
        assert "k_batch_pq_" not in src, f                                   # the launches themselves are the new file's
        for m in re.finditer(r"MGF_TRY\(batch_pq_[^\n]*\n", src):          # each stands where the launch it replaces follows as the else
            assert src[m.end():].lstrip().startswith("else "), (f, m.group(0))
    for f in ("host_batch_camera.inc", "host_batch_touch.inc", "host_batch_drive.inc", "host_batch_rollout.inc"):
        assert "batch_pq_" not in read("mgf_amd", "csrc", f), f


def test_the_kernels_source():
    k = read("mgf_amd", "csrc", "k_batch_part_query.h")
    names = set(re.findall(r"void (k_batch_\w+)\(", k))
    assert names == {"k_batch_pq_ray", "k_batch_pq_sensor", "k_batch_pq_sweep", "k_batch_pq_feeler", "k_batch_pq_overlap", "k_batch_pq_zone", "k_batch_pq_nearest"}
    assert not any(n.startswith(p) for n in names for p in QC.PINNED_PREFIXES)
    for word in ("WHY THE BODY-LEVEL REJECT CHANGES NO ANSWER", "bq_ray_far", "q_sweep_far", "RB >= |m_k - C| + ra_k", "min(count, kMaxParts)",
                 "36 bytes a body", "there is no persistent row"):
        assert word in k, word
    # `part` travels: the candidate of the ray front carries it through shfl, pack, unpack and merge
    best = k[k.index("struct PartBest : QueryBest"):k.index("// col0 / col1 of an ordinary body")]
    assert "o.part = (uint32_t)__shfl_xor((int)part, off)" in best and "u2f(part)" in best and "o.part = f2u(r0.w)" in best and "o.index, o.part)" in best
    # the part walks are the policy's (PartBodies), and the ray front's candidate is the policy's type
    policy = k[k.index("struct PartBodies {"):k.index("void k_batch_pq_ray(")]
    ray = policy[policy.index("PartBest ray_walk("):policy.index("SweepBest sweep_walk(")]
    assert "using Best = PartBest;" in policy and "PartBest best;" in ray and "best.offer(ip, t, MGF_HIT_BODY, i, k)" in ray
    sweep = policy[policy.index("SweepBest sweep_walk("):policy.index("Box box(")]
    assert sweep.count("comp_mcomp(") == 1 and "best.offer(ct, MGF_HIT_BODY, i, k, 0u)" in sweep and "scalar" in sweep and "ONE loop over (body i, part k)" in sweep
    assert "pq_stage(A, P, g0, n, " in policy and not re.search(r"return;|__syncthreads|atomic", policy)
    # the fronts' barrier discipline: one exit ahead of the staging (a whole workgroup), one behind the reduction - on the fronts the
    # existing kernels share with these (k_batch_query.h): one text serves both
    q = read("mgf_amd", "csrc", "k_batch_query.h")
    for a in ("void bq_ray_front(", "void bq_sweep_front("):
        body = q[q.index(a):]
        body = body[:body.index("\n}\n")]
        assert body.count("return;") == 2 and body.index("return;") < body.index("bodies.stage(") < body.index("bq_reduce(") < body.rindex("return;")
        assert "__syncthreads" not in body                                 # (the barriers are the staging's and bq_reduce's)
    assert "typename Bodies::Best best;" in q[q.index("void bq_ray_front("):q.index("void bq_ray_item(")]
    stage = k[k.index("void pq_stage("):k.index("// the body-level rejects")]
    assert stage.count("__syncthreads()") == 1 and stage.rstrip().endswith("__syncthreads();\n}") and "return" not in stage
    # the box front is k_batch_observe.h's own: nothing of it stands here, only a body's box
    for text in ("bo_front", "__ballot(", "min(W.shift(), 6u)", "box_overlaps("):
        assert text not in k[k.index("#pragma once"):], text
    o = read("mgf_amd", "csrc", "k_batch_observe.h")
    box = o[o.index("uint32_t bo_front("):o.index("void bo_overlap(")]
    assert "return;" not in box and box.count("__syncthreads()") == 1 and "__ballot(hit)" in box and "bodies.box((size_t)g0 + i)" in box
    assert "Box box(size_t g) const { return pq_body_box(A, P, g); }" in policy
    # every kernel is one call of the body it shares with the existing kernel
    for call in ("bq_ray_item<SRC>(A, PartBodies(A, P), ", "bs_rays(A, PartBodies(A, P), ", "bq_sweep_item<SRC>(A, PartBodies(A, P), ", "bf_casts(A, PartBodies(A, P), ",
                 "bo_overlap<FILL>(A, PartBodies(A, P), ", "bz_first<SRC>(A, PartBodies(A, P), ", "bn_nearest<SRC>(A, PartBodies(A, P), "):
        assert k.count(call) == 1, call
    # the existing kernels' sources are not the place of a new kernel
    for f in ("k_batch_query.h", "k_batch_query_dev.h", "k_batch_sensor.h", "k_batch_feeler.h", "k_batch_zone.h", "k_batch_nearest.h", "k_batch_observe.h"):
        assert "pq_" not in read("mgf_amd", "csrc", f), f


def test_compiler_figures_no_scratch_no_spills_and_design_records_them():
    rows = kernel_resources("k_batch_pq_")
    assert set(rows) == QC.NEW_KERNELS, sorted(rows)
    design = read("DESIGN.md")
    for name in sorted(rows):
        vgpr, sgpr, scratch, lds, sspill, vspill = rows[name]
        print(name, rows[name])
        assert (scratch, lds, sspill, vspill) == ("0", "0", "0", "0"), (name, rows[name])
        assert "`%s` %s / %s / 0 / 0 / 0" % (name, vgpr, sgpr) in design, (name, rows[name])
    everything = kernel_resources("k_batch_")
    for prefix in QC.PINNED_PREFIXES:
        assert not any(n.startswith(prefix) and "pq" in n for n in everything), prefix


def test_documents():
    design = read("DESIGN.md")
    sec = design[design.index("### Part queries"):]
    for word in ("part_queries", "k_batch_part_query.h", "host_batch_part_query.inc", "reject sphere", "PartBest", "mgf_batch_cast_cameras(_dev)` stay refused",
                 "batch_part_query_bench.py", "Compiler output"):
        assert word in sec, word
    for f in ("README.md", "INTEGRATION.md"):
        assert "part_queries" in read(f), f


def test_the_python_wrapper_takes_the_option():
    import mgf_amd
    src = inspect.getsource(mgf_amd.WorldBatch.set_option)
    assert "mgf_batch_set_option" in src and "key.encode()" in src and "int(value)" in src
    doc = mgf_amd.WorldBatch.set_option.__doc__ or ""
    assert '"part_queries" (0 | 1)' in doc and "the cameras do not" in doc
    assert QC.OPTION == "part_queries" and len(QC.IN_SCOPE) == 9
    h = read("include", "mgf_hip.h")
    for call in QC.IN_SCOPE:
        assert call in h, call
