"""Scenes, rays and helpers for the batch's part-aware queries (option "part_queries"): tests/test_world_batch_part_queries_host.py and
tests/test_gpu_world_batch_part_queries.py.  The scenes are tests.batch_parts_cases' - at most 218 bodies a world - and a call holds a
few hundred queries."""
import numpy as np

from mgf_amd import scenes
from tests import batch_parts_cases as PC

f32 = np.float32
OPTION = "part_queries"
# rays (and casts) per world of the six scenes in one shuffled call: 300 -> two work items (256 + 44: 1 and 4 lanes a query), 70 -> 2
# lanes, 3 -> 64 lanes, 1 -> 256 lanes.  (A world must show more than 32 hits on its bodies of several components, so the counts 1 and 3
# go to the worlds without such bodies; the GPU tests send one and three queries of every world WITH them in calls of their own.)
COUNTS = {PC.DUMBBELLS: 300, PC.JACKS: 70, PC.PILE: 3, PC.MIXED: 70, PC.EMPTY: 1, PC.ONE_JACK: 70}
NEW_KERNELS = {"k_batch_pq_ray<0>", "k_batch_pq_ray<1>", "k_batch_pq_ray<2>", "k_batch_pq_sweep<0>", "k_batch_pq_sweep<1>", "k_batch_pq_sweep<2>",
               "k_batch_pq_sensor", "k_batch_pq_feeler", "k_batch_pq_overlap<false>", "k_batch_pq_overlap<true>", "k_batch_pq_zone<0>",
               "k_batch_pq_zone<2>", "k_batch_pq_nearest<0>", "k_batch_pq_nearest<2>"}
PINNED_PREFIXES = ("k_batch_sensor_", "k_batch_camera_", "k_batch_zone_", "k_batch_feeler", "k_batch_query_")
IN_SCOPE = ("mgf_batch_raycast_many", "mgf_batch_sweep_many", "mgf_batch_cast_sensors", "mgf_batch_cast_feelers", "mgf_batch_overlap_aabb_many",
            "mgf_batch_overlap_first_dev", "mgf_batch_overlap_nearest_dev", "mgf_batch_read_zones", "mgf_batch_read_zones_nearest")


def compound_parts(sc):
    """body index -> the COMPONENT_DTYPE rows of its parts as added (tick 0), for the bodies of several components of a scene"""
    cb = sc.get("compound")
    if cb is None:
        return {}
    n0, off = len(sc["comps"]), cb["offsets"]
    return {n0 + b: cb["comps"][off[b]:off[b + 1]] for b in range(len(off) - 1)}


def centres(rows):
    """the middle of every component of COMPONENT_DTYPE / MOVING_DTYPE rows"""
    return np.asarray(rows["p"], np.float64) + 0.5 * np.asarray(rows["d"], np.float64) * (np.asarray(rows["tag"]) == 1)[:, None]


def rotate(q, v):
    """Rotation::rotate_vector for q = (s, x, y, z), in f64: where to aim, never what to compare"""
    s, u = float(q[0]), np.asarray(q[1:], np.float64)
    v = np.asarray(v, np.float64)
    return v + 2.0 * s * np.cross(u, v) + 2.0 * np.cross(u, np.cross(u, v))


def aim_points(sc, x0, st):
    """points to aim at: the middles of the parts of the scene's bodies of several components where the state `st` has carried them
    (x0: the bodies' x at tick 0, when the parts were where the scene put them), and the centres of its ordinary bodies"""
    pts = [np.asarray(st["x"][:len(sc["comps"])], np.float64)]
    for i, rows in compound_parts(sc).items():
        local = centres(rows) - np.asarray(x0[i], np.float64)
        pts.append(np.asarray(st["x"][i], np.float64) + np.array([rotate(st["q"][i], v) for v in local]))
    return np.concatenate(pts) if pts else np.zeros((0, 3))


def tie_scene():
    """two identical bodies at the same place, each two spheres of radius 0.5 at (+-0.25, 1, 0); no terrain, no gravity"""
    base = PC.empty_scene(None)
    comps = np.zeros(4, scenes.COMPONENT_DTYPE)
    comps["tag"], comps["r"] = 0, 0.5
    comps["p"] = [(-0.25, 1, 0), (0.25, 1, 0), (-0.25, 1, 0), (0.25, 1, 0)]
    cb = dict(comps=comps, comp_mass=np.ones(4, f32), offsets=np.array([0, 2, 4], np.int64), restitution=np.zeros(2, f32),
              friction=np.full(2, 0.5, f32), force=np.zeros((2, 3), f32))
    return dict(base, name="ties", compound=cb)


def shuffled(rng, world, *arrays):
    """one call's queries of several worlds in a seeded random order"""
    perm = rng.permutation(len(world))
    return (np.ascontiguousarray(world[perm]),) + tuple(np.ascontiguousarray(a[perm]) for a in arrays)
