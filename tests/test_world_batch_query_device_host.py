"""The device-pointer ray casts and sweeps of a batch (mgf_batch_raycast_many_dev, mgf_batch_sweep_many_dev) without a GPU: the header
declares them and the plan's launch constant and no longer leaves them out, the library, the binding and INTEGRATION.md carry them,
what can be refused before a device is looked at is refused there, host_batch_query_dev.inc looks every pointer up before it enqueues
anything, the binding turns down a tensor of the wrong kind before it calls C, the new kernels and the three guarded ones use no
scratch and spill nothing - and the plan the device builds, modelled in numpy over the GPU tests' own world arrays, is a partition."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mgf_amd
from mgf_amd import _capi
from tests import batch_query_device_cases as QD
from tests.util import ROOT, kernel_resources, read

ENTRY_POINTS = {
    "mgf_batch_raycast_many_dev": r"mgf_status mgf_batch_raycast_many_dev\(mgf_batch\* b, const int32_t\* world_dev, const mgf_particle\* parts_dev, int64_t n,\s*"
                                  r"const int32_t\* ignore_body_dev, int32_t kinds_mask, mgf_ray_hit\* out_dev\);",
    "mgf_batch_sweep_many_dev": r"mgf_status mgf_batch_sweep_many_dev\(mgf_batch\* b, const int32_t\* world_dev, const mgf_moving_component\* casts_dev, int64_t n,\s*"
                                r"const int32_t\* ignore_body_dev, int32_t kinds_mask, mgf_sweep_hit\* out_dev\);",
}
NEW_KERNELS = {"k_batch_query_plan_count<7u>", "k_batch_query_plan_count<13u>", "k_batch_query_plan_cut", "k_batch_query_plan_fill",
               "k_batch_query_ray_dev<1>", "k_batch_query_ray_dev<2>", "k_batch_query_sweep_bodies_dev<1>", "k_batch_query_sweep_bodies_dev<2>"}
GUARDED = {"k_batch_query_sweep_faces", "k_batch_query_ray_obstacles", "k_batch_query_sweep_obstacles"}


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_integration_md_carry_the_calls():
    h = read("include", "mgf_hip.h")
    for name, sig in ENTRY_POINTS.items():
        assert re.search(r"MGF_API " + sig, h), name
    section = h[h.index("device-pointer calls"):]
    m = re.search(r"#define MGF_BATCH_DEV_QUERY_PLAN_LAUNCHES (\d+)", section)
    assert m and int(m.group(1)) == _capi.BATCH_DEV_QUERY_PLAN_LAUNCHES and 2 <= int(m.group(1)) <= 3
    # what is left out: the sentence no longer names rays and sweeps, and still names the rest
    out = re.sub(r"\s*\n \*\s*", " ", section[section.index("OUT OF SCOPE here:"):section.index("#define MGF_BATCH_DEV_SET_LAUNCHES")])
    assert "device-pointer rays" not in out and "sweeps" not in out and "sort by world is on the host" not in out
    for word in ("device-pointer box queries", "CSR total", "rays given in a body's frame", "hipGraph", "lone mgf_world"):
        assert word in out, word
    for word in ("world_dev == NULL", "multiple of n_worlds", "device_skipped", "no-hit record", "nothing enqueued", "overlapping", "lane scheduling",
                 "No float atomic", "\"query_run_ns\" is 0", "28 n", "44 n", "52 n"):
        assert word in section, word
    lib = mgf_amd.load_library()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
    for name in ENTRY_POINTS:
        assert name in _capi.SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32 and list(fn.argtypes) == [vp, vp, vp, i64, vp, i32, vp], name
    for method in ("raycast_dev", "sweep_dev"):
        assert callable(getattr(mgf_amd.WorldBatch, method)), method
    flat = re.sub(r"\s+", " ", read("INTEGRATION.md"))
    for sig in ("pub fn mgf_batch_raycast_many_dev(b: *mut mgf_batch, world_dev: *const i32, parts_dev: *const mgf_particle, n: i64, "
                "ignore_body_dev: *const i32, kinds_mask: i32, out_dev: *mut mgf_ray_hit) -> mgf_status;",
                "pub fn mgf_batch_sweep_many_dev(b: *mut mgf_batch, world_dev: *const i32, casts_dev: *const mgf_moving_component, n: i64, "
                "ignore_body_dev: *const i32, kinds_mask: i32, out_dev: *mut mgf_sweep_hit) -> mgf_status;"):
        assert sig in flat, sig
    kernels = read("mgf_amd", "csrc", "kernels.h")
    assert '#include "k_batch_query_dev.h"' in kernels and "k_batch_query_plan_count" in kernels
    hip = read("mgf_amd", "csrc", "mgf_hip.hip")
    assert hip.index('#include "host_batch_query.inc"') < hip.index('#include "host_batch_dev.inc"') < hip.index('#include "host_batch_query_dev.inc"')
    design = read("DESIGN.md")
    sub = design[design.index("Device-pointer queries"):]
    for word in ("k_batch_query_plan_count", "k_batch_query_plan_fill", "lane scheduling", "batch_device_query_bench.py"):
        assert word in sub, word
    assert "raycast_dev" in read("README.md") and "sweep_dev" in read("README.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "batch_device_query_bench.py"))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_what_needs_no_device_is_refused_before_the_handle_is_dereferenced():
    lib = mgf_amd.load_library()
    INV = _capi.ERR_INVALID

    def err():
        return lib.mgf_last_error().decode()
    fake = C.c_void_p(16)   # a handle that is never dereferenced, "device" addresses that are never looked up
    dev, out = C.c_void_p(4096), C.c_void_p(1 << 20)
    for name in ENTRY_POINTS:
        fn = getattr(lib, name)
        assert fn(None, dev, dev, 4, dev, 7, out) == INV and "NULL" in err(), name
        assert fn(fake, dev, dev, -1, dev, 7, out) == INV and "negative" in err(), name
        assert fn(fake, dev, dev, -(1 << 40), dev, 7, out) == INV and "negative" in err(), name
        assert fn(fake, dev, dev, 1 << 31, dev, 7, out) == INV and "too many" in err(), name
        assert fn(fake, dev, None, 4, dev, 7, out) == INV and "NULL" in err(), name
        assert fn(fake, dev, dev, 4, dev, 7, None) == INV and "NULL" in err(), name
        assert fn(fake, None, None, 4, None, 7, out) == INV and "NULL" in err(), name
        for mask in (0, 8, -1, 16):
            assert fn(fake, dev, dev, 4, dev, mask, out) == INV and "kinds_mask" in err(), (name, mask)
            assert fn(fake, dev, dev, 0, dev, mask, out) == INV and "kinds_mask" in err(), (name, mask)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_every_device_pointer_is_looked_up_before_the_first_enqueue():
    """the order "check, then enqueue", read in the source: in host_batch_query_dev.inc - both entry points are one line each into
    batch_query_dev_run - the last dev_span and the overlap check come before the first thing that enqueues (a push of the mirror, an
    upload of a table, a memset, a copy, a launch, a prefix sum), and the refusals that need no device before the handle is read"""
    src = read("mgf_amd", "csrc", "host_batch_query_dev.inc")
    parts = re.split(r"\n(?=extern \"C\"|template <class Q>\nstatic mgf_status batch_query_dev_run)", src)
    assert len(parts) == 4, len(parts)
    run, entries = parts[1], parts[2:]
    for e in entries:
        assert "return batch_query_dev_run(" in e and not re.search(r"dev_span|<<<|Async|batch_push|batch_dev_begin", e), e[:100]
    enqueue = (r"batch_ray_obstacles\(|batch_sweep_tail\(|batch_push\(|batch_dev_begin\(|batch_env_sync\(|batch_cols_refresh\(|hipMemsetAsync|hipMemcpyAsync|<<<|"
               r"prim_exclusive_scan_u32|\.ensure\(")
    first_enqueue = min(m.start() for m in re.finditer(enqueue, run))
    checks = [m.start() for m in re.finditer(r"dev_span\(", run)]
    assert len(checks) == 4 and max(checks) < first_enqueue
    for name in ("world_dev, 4 \\* n", "q_dev, sizeof\\(Q\\) \\* n", "ignore_dev, 4 \\* n", "out_dev, 4 \\* kOut \\* n"):
        assert re.search(r"dev_span\(b->ctx, " + name, run), name
    # out_dev, the one array written, against each of the three inputs (which may share bytes among themselves): the one helper over
    # the list, ahead of the first enqueue, with the message as it was
    listed = run.index('arrays[4] = {{out_dev, 4 * kOut * n, "out_dev"}, {world_dev, 4 * n, "world_dev"}, {q_dev, sizeof(Q) * n, "q_dev"}, '
                       '{ignore_dev, 4 * n, "ignore_dev"}};')
    overlap = run.index('dev_outputs_overlap(arrays, 4, 1, "an input array")')
    assert max(checks) < listed < overlap < first_enqueue and run.count("dev_outputs_overlap(") == 1
    assert run.index("out_dev overlaps an input array") < first_enqueue
    helper = parts[0][parts[0].index("static mgf_status dev_outputs_overlap("):]
    assert "dev_bytes_overlap(a[i].p, a[i].bytes, a[j].p, a[j].bytes)" in helper and "for (size_t j = i + 1; j < n; ++j)" in helper
    assert '"%s overlaps %s", a[i].name, j < n_out || !inputs ? a[j].name : inputs' in helper
    assert not re.search(enqueue, helper) and "b->" not in helper
    # before the handle is read: NULL batch / n (batch_dev_args), NULL arrays, the mask
    first_deref = run.index("b->")
    for early in ("batch_dev_args(b, n_in)", "\"NULL argument\"", "query_mask_check(kinds_mask)"):
        assert run.index(early) < first_deref, early
    # n = 0 launches nothing: it returns before the first enqueue
    assert run.index("if (n == 0) return MGF_OK;") < first_enqueue
    k = read("mgf_amd", "csrc", "k_batch_query_dev.h")
    count = k[k.index("void k_batch_query_plan_count"):k.index("void k_batch_query_plan_cut")]
    assert count.index("(uint32_t)w < A.K") < count.index("A.cnt[w]") and "atomicAdd(A.skipped, 1ull)" in count
    assert not re.search(r"atomic\w*\((?![^;]*(skipped|cnt))", k), "an atomic on anything but the integer counters"
    q = read("mgf_amd", "csrc", "k_batch_query.h")
    for kernel in GUARDED:
        body = q[q.index("void " + kernel + "("):]
        body = body[:body.index("\n}\n")]
        assert body.index("if (w < 0) return;") < min(body.index("tdesc[") if "tdesc[" in body else 1 << 30, body.index("batch_terrain_of(") if "batch_terrain_of(" in body else 1 << 30), kernel
        assert "world[i]" not in body, kernel
    for item in ("bq_ray_front", "bq_sweep_front"):   # (bq_ray_item<SRC> / bq_sweep_item<SRC> are these over the caller's particles / casts)
        body = q[q.index("void " + item + "("):]
        assert body.index("blockIdx.x >= *S.n_items) return;") < body.index("bodies.stage(") < body.index("\n}\n"), item
    wrapper = q[q.index("void bq_ray_item("):q.index("void k_batch_query_ray(")]
    assert "bq_ray_front<SRC>(" in wrapper and not re.search(r"return;|__syncthreads|atomic", wrapper)
    wrapper = q[q.index("void bq_sweep_item("):q.index("void k_batch_query_sweep_bodies(")]
    assert "bq_sweep_front<SRC>(" in wrapper and not re.search(r"return;|__syncthreads|atomic", wrapper)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_binding_turns_a_wrong_tensor_down_before_it_calls_c():
    import torch

    class Handle(mgf_amd.WorldBatch):   # no context, no C handle: a call that got as far as C would fail differently
        def __init__(self):
            self._h, self.n_worlds = None, 2

    b = Handle()
    n = 4
    # raw addresses pass as they are, so every call below gets as far as its one tensor - and no further: with no handle C would refuse
    addr = dict(world=4096, out=1 << 20, ignore=1 << 21, n=n)
    right = dict(world=torch.zeros(n, dtype=torch.int32), ignore=torch.zeros(n, dtype=torch.int32),
                 parts=torch.zeros((n, 7), dtype=torch.float32), casts=torch.zeros((n, 11), dtype=torch.float32))
    wrong = {
        "world": [torch.zeros(n, dtype=torch.int64), torch.zeros(2 * n, dtype=torch.int32)[::2], torch.zeros(n + 1, dtype=torch.int32)],
        "ignore": [torch.zeros(n, dtype=torch.float32), torch.zeros(n - 1, dtype=torch.int32), torch.zeros(2 * n, dtype=torch.int32)[::2]],
        "parts": [torch.zeros((n, 7), dtype=torch.float64), torch.zeros((7, n), dtype=torch.float32).t(), torch.zeros((n, 6), dtype=torch.float32),
                  torch.zeros((n, 7), dtype=torch.int32), torch.zeros((n + 1, 7), dtype=torch.float32)],
        "casts": [torch.zeros((n, 11), dtype=torch.float64), torch.zeros((n, 7), dtype=torch.float32), torch.zeros((11, n), dtype=torch.int32).t(),
                  torch.zeros((n - 1, 11), dtype=torch.int32)],
    }
    wrong_out = {7: [torch.zeros((n, 7), dtype=torch.float32), torch.zeros((n, 13), dtype=torch.int32), torch.zeros((n + 1, 7), dtype=torch.int32),
                     torch.zeros((7, n), dtype=torch.int32).t()],
                 13: [torch.zeros((n, 7), dtype=torch.int32), torch.zeros((n, 13), dtype=torch.float32), torch.zeros((13, n), dtype=torch.int32).t()]}
    for call, q, cols in ((b.raycast_dev, "parts", 7), (b.sweep_dev, "casts", 11)):
        good = dict(addr, **{q: 8192})
        outs = 7 if q == "parts" else 13
        for key in ("world", "ignore", q, "out"):
            for t in (wrong_out[outs] if key == "out" else wrong[key]):
                with pytest.raises(ValueError) as e:
                    call(**dict(good, **{key: t}))
                assert "on cpu" not in str(e.value), (key, str(e.value))        # turned down for what it is, not for where it is
            t = torch.zeros((n, outs), dtype=torch.int32) if key == "out" else right[key]
            with pytest.raises(ValueError, match="on cpu"):                      # everything right but the device
                call(**dict(good, **{key: t}))
        with pytest.raises(ValueError):                                          # the queries and out are required
            call(**dict(good, out=None))
        with pytest.raises(ValueError):
            call(**dict(good, **{q: None}))
        with pytest.raises(ValueError, match="n must be given"):                 # a raw address needs n
            call(**dict(good, n=None))
        with pytest.raises(ValueError, match="not ndarray"):                     # neither a tensor nor an address
            call(**dict(good, **{q: np.zeros((n, cols), np.float32)}))
        with pytest.raises(ValueError, match="multiple"):                        # the fixed layout: n is a multiple of n_worlds
            call(**dict(good, world=None, n=3))
    with pytest.raises(ValueError, match="on cpu"):          # int32 words are a cast's other dtype; it gets as far as the device check
        b.sweep_dev(4096, torch.zeros((n, 11), dtype=torch.int32), 1 << 20)
    with pytest.raises(mgf_amd.MgfError):                    # and a call whose arguments are all in order does reach C
        b.raycast_dev(**dict(addr, parts=8192))


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_new_and_the_guarded_kernels_use_no_scratch_and_spill_nothing():
    if not os.path.exists(os.path.join(ROOT, "mgf_amd", "libmgf_hip.so")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    rows = kernel_resources("k_batch_query_")
    assert NEW_KERNELS | GUARDED <= set(rows), sorted(rows)
    bad = {k: v for k, v in rows.items() if k in NEW_KERNELS | GUARDED and (v[2], v[4], v[5]) != ("0", "0", "0")}
    assert not bad, bad
    # the kernels of the host-memory calls and their device-pointer twins are one piece of code: the same static LDS, about the same registers
    for host, dev in (("k_batch_query_ray", "k_batch_query_ray_dev"), ("k_batch_query_sweep_bodies", "k_batch_query_sweep_bodies_dev")):
        for src in (1, 2):
            twin = rows[f"{dev}<{src}>"]
            assert twin[3] == rows[host][3] and int(twin[0]) <= int(rows[host][0]) + 8, (dev, src, twin, rows[host])
    k = read("mgf_amd", "csrc", "k_batch_query_dev.h")
    assert len(re.findall(r"__global__ __launch_bounds__\(kBatchBlock\)", k)) == len(re.findall(r"__global__", k)) == 5


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
def _plan_cases():
    pile = QD.pile_world_array()
    K = len(QD.PILE_BODIES)
    bad = QD.bad_worlds(K)
    at = QD.skip_positions(len(pile), len(bad))
    with_bad, keep = QD.spread(dict(world=pile), dict(world=bad), at)
    one_each, all_last = QD.many_world_arrays()
    return [("pile", pile, K, 0), ("pile reversed", pile[::-1], K, 0), ("pile with skipped records", with_bad["world"], K, len(bad)),
            ("one ray a world", one_each, QD.MANY, 0), ("every ray to the last world", all_last, QD.MANY, 0)]


@pytest.mark.parametrize("case", range(5))
def test_the_plan_is_a_partition_into_items_of_at_most_256(case):
    name, world, K, n_bad = _plan_cases()[case]
    n = len(world)
    items, order, skipped = QD.plan_model(world, K)
    assert skipped == n_bad, name
    valid = np.flatnonzero((world >= 0) & (world < K))
    assert sorted(order.tolist()) == valid.tolist(), name                      # every valid query exactly once, no other
    assert np.all(items >= 0) and len(items) <= n // 256 + min(n, K), (name, len(items))
    seen = np.zeros(n, np.int64)
    for w, first, count in items:
        assert 1 <= count <= 256, (name, count)
        q = order[first:first + count]
        assert np.all(world[q] == w), name                                     # an item holds queries of its own world only
        seen[q] += 1
    assert np.all(seen[valid] == 1) and seen.sum() == len(valid), name         # every valid query in exactly one item
    assert np.all(np.diff(items[:, 0]) >= 0) and np.all(np.diff(items[:, 1]) > 0), name   # the order BatchQueryPlan::fill writes them in
    counts = np.bincount(world[valid].astype(np.int64), minlength=K)
    assert len(items) == int(np.sum((counts + 255) // 256)), name
    if name == "pile":
        assert counts.tolist() == [3, 64, 300, 0, 257] and len(items) == 1 + 1 + 2 + 0 + 2
    if name == "every ray to the last world":
        assert items.tolist() == [[QD.MANY - 1, 0, 256], [QD.MANY - 1, 256, 44]]
    if name == "one ray a world":
        assert len(items) == QD.MANY > 256 and np.all(items[:, 2] == 1)


# ---- the GPU tests' inputs, without a GPU -------------------------------------------------------------------------------------------------
def test_rays_of_the_obstacle_world_meet_its_ring_first():
    """by the oracle alone: after the 30 ticks no body of the obstacle's world has met the ring (its list changes nothing of the tick),
    and rays of BQ.pile_rays meet the ring ahead of every body - so the obstacle pass of the GPU tests has something to answer"""
    from oracle import oracle as O
    from tests import batch_obstacle_cases as BC
    from tests import batch_query_cases as BQ
    from tests.util import oracle_world
    sc = QD.pile_scenes()[QD.OBSTACLE_WORLD]
    with_ring, without = BC.oracle_with_obstacles(sc), oracle_world(sc)
    for _ in range(QD.TICKS):
        with_ring.step(float(sc["dt"]), sc["iters"])
        without.step(float(sc["dt"]), sc["iters"])
    x = np.asarray(with_ring.state()["x"])
    assert x.tobytes() == np.asarray(without.state()["x"]).tobytes()
    cen = [np.zeros((c, 3)) for c in QD.PILE_BODIES]
    cen[QD.OBSTACLE_WORLD] = x
    rays = BQ.pile_rays(cen, BQ.COUNTS_T30)
    sel = rays["world"] == QD.OBSTACLE_WORLD
    ring = BC.oracle_compounds([QD.RING])[0]
    r = float(sc["comps"]["r"][0])
    first = 0
    for p, d, dt in zip(rays["p"][sel], rays["d"][sel], rays["dt"][sel]):
        h = ring.intersection(p, d, float(dt)) if np.any(d) else None
        if h is None:
            continue
        tb = [O.intersection(p, d, float(dt), O.shape(O.SPHERE, c.astype(np.float32), r)) for c in x]
        first += all(b is None or h[1] < b[1] for b in tb)
    assert first >= 2, first
    # and the casts of the world without bodies meet its ring: Compound::contacts of the swept shape reports a contact
    low = BC.oracle_compounds([QD.LOW_RING])[0]
    met = []
    for c in QD.empty_world_casts():
        sh = O.shape(O.SPHERE, c["p"], float(c["r"])) if c["tag"] == 0 else O.shape(O.CAPSULE, c["p"], c["d"], float(c["r"]))
        met.append(len(low.contacts(sh, c["delta"])) > 0)
    assert met == [True, True, False, False], met
