"""ctypes binding of include/mgf_hip.h.  Names follow the reference (mgf) API they replace."""
import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    # (MGF_AMD_LIB: a differently built libmgf_hip.so for an A/B experiment; never a different implementation)
    return os.environ.get("MGF_AMD_LIB") or os.path.join(_HERE, "libmgf_hip.so")


class MgfError(RuntimeError):
    """A non-OK mgf_status; `.status` holds the code (the reference panics in these cases)."""

    def __init__(self, status, msg):
        super().__init__(f"mgf status {status} ({_STATUS_NAMES.get(status, '?')}): {msg}")
        self.status = status


_STATUS_NAMES = {0: "OK", 1: "EMPTY", 2: "NOT_OCCUPIED", 3: "NOT_LEAF", 4: "STATIC_REF", 5: "SINGULAR", 6: "INVALID",
                 7: "CAPACITY", 8: "HIP", 9: "OOM"}
OK, ERR_EMPTY, ERR_NOT_OCCUPIED, ERR_NOT_LEAF, ERR_STATIC_REF, ERR_SINGULAR, ERR_INVALID, ERR_CAPACITY, ERR_HIP, ERR_OOM = range(10)
SPHERE, CAPSULE, TRIANGLE, RECTANGLE, PLANE, RAY, SEGMENT, AABB = 0, 1, 2, 3, 4, 5, 6, 7


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def tup(self):
        return (self.x, self.y, self.z)


class Quat(C.Structure):
    _fields_ = [("s", C.c_float), ("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Aabb(C.Structure):
    _fields_ = [("c", Vec3), ("r", Vec3)]


class BatchSensor(C.Structure):
    _fields_ = [("world", C.c_int32), ("body", C.c_int32), ("p", Vec3), ("d", Vec3), ("dt", C.c_float), ("flags", C.c_int32)]


class BatchCamera(C.Structure):
    _fields_ = [("world", C.c_int32), ("body", C.c_int32), ("p", Vec3), ("r", C.c_float * 4), ("tan_x", C.c_float), ("tan_y", C.c_float),
                ("far", C.c_float), ("width", C.c_int32), ("height", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class BatchZone(C.Structure):
    _fields_ = [("world", C.c_int32), ("body", C.c_int32), ("p", Vec3), ("r", Vec3), ("flags", C.c_int32), ("reserved", C.c_int32)]


class BatchFeeler(C.Structure):
    _fields_ = [("world", C.c_int32), ("body", C.c_int32), ("tag", C.c_int32), ("flags", C.c_int32), ("p", Vec3), ("d", Vec3), ("r", C.c_float),
                ("delta", Vec3), ("reserved", C.c_int32 * 2)]


class BatchActuator(C.Structure):
    _fields_ = [("world", C.c_int32), ("body", C.c_int32), ("flags", C.c_uint32), ("gain", C.c_float), ("p", Vec3), ("lo", C.c_float),
                ("d", Vec3), ("hi", C.c_float)]


class BatchSpring(C.Structure):
    _fields_ = [("world", C.c_int32), ("body", C.c_int32), ("other", C.c_int32), ("flags", C.c_uint32), ("pa", Vec3), ("rest", C.c_float),
                ("pb", Vec3), ("k", C.c_float), ("c", C.c_float), ("lo", C.c_float), ("hi", C.c_float), ("pad", C.c_float)]


class BatchJoint(C.Structure):
    _fields_ = [("world", C.c_int32), ("body", C.c_int32), ("other", C.c_int32), ("flags", C.c_uint32), ("pa", Vec3), ("beta", C.c_float),
                ("pb", Vec3), ("pad", C.c_float)]


class BatchHinge(C.Structure):
    _fields_ = [("world", C.c_int32), ("body", C.c_int32), ("other", C.c_int32), ("flags", C.c_uint32), ("pa", Vec3), ("beta", C.c_float),
                ("pb", Vec3), ("tmax", C.c_float), ("ax", Vec3), ("cm", C.c_float), ("ua", Vec3), ("sm", C.c_float),
                ("bx", Vec3), ("ch", C.c_float), ("ub", Vec3), ("sh", C.c_float)]


class BatchSlider(C.Structure):
    _fields_ = [("world", C.c_int32), ("body", C.c_int32), ("other", C.c_int32), ("flags", C.c_uint32), ("pa", Vec3), ("beta", C.c_float),
                ("pb", Vec3), ("fmax", C.c_float), ("ax", Vec3), ("lo", C.c_float), ("ua", Vec3), ("hi", C.c_float),
                ("bx", Vec3), ("pad0", C.c_float), ("ub", Vec3), ("pad1", C.c_float)]


class Component(C.Structure):
    _fields_ = [("tag", C.c_int32), ("p", Vec3), ("d", Vec3), ("r", C.c_float)]


class MovingComponent(C.Structure):
    _fields_ = [("shape", Component), ("delta", Vec3)]


class Shape(C.Structure):
    _fields_ = [("kind", C.c_int32), ("v", C.c_float * 12)]


class Contact(C.Structure):
    _fields_ = [("a", Vec3), ("b", Vec3), ("n", Vec3), ("t", C.c_float)]


class LocalContact(C.Structure):
    _fields_ = [("local_a", Vec3), ("local_b", Vec3), ("glob", Contact)]


class BodyRef(C.Structure):
    _fields_ = [("tag", C.c_int32), ("index", C.c_uint32), ("center", Vec3), ("friction", C.c_float)]


class Velocity(C.Structure):
    _fields_ = [("linear", Vec3), ("angular", Vec3)]


class RigidBodyInfo(C.Structure):
    _fields_ = [("x", Vec3), ("restitution", C.c_float), ("friction", C.c_float), ("inv_mass", C.c_float),
                ("inv_moment", C.c_float * 9)]


class Params(C.Structure):
    _fields_ = [("baumgarte", C.c_float), ("penetration_slop", C.c_float), ("persistent_threshold_sq", C.c_float),
                ("collision_epsilon", C.c_float), ("fat_margin", C.c_float)]


class StepStats(C.Structure):
    _fields_ = [("n_bodies", C.c_uint64), ("n_constraints", C.c_uint64), ("n_terrain_constraints", C.c_uint64),
                ("n_pair_candidates", C.c_uint64), ("n_terrain_candidates", C.c_uint64), ("n_refits", C.c_uint64),
                ("n_levels", C.c_uint32), ("iters", C.c_uint32),
                ("ms_integrate", C.c_float), ("ms_broadphase", C.c_float), ("ms_narrowphase", C.c_float),
                ("ms_setup", C.c_float), ("ms_solve", C.c_float), ("ms_total", C.c_float),
                ("solver_kernel_launches", C.c_uint64), ("ms_solver_kernels", C.c_float), ("n_ghost_constraints", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    def __getitem__(self, key):  # a read-only mapping view: callers in a hot loop need not build the dict
        return getattr(self, key)


COMPONENT_DTYPE = np.dtype([("tag", "<i4"), ("p", "<f4", 3), ("d", "<f4", 3), ("r", "<f4")])
MOVING_DTYPE = np.dtype([("tag", "<i4"), ("p", "<f4", 3), ("d", "<f4", 3), ("r", "<f4"), ("delta", "<f4", 3)])
CONSTRAINT_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("n_contacts", "<i4"),
                             ("normal", "<f4", 3), ("t0", "<f4", 3), ("t1", "<f4", 3), ("ra", "<f4", 3), ("rb", "<f4", 3),
                             ("bias", "<f4"), ("normal_mass", "<f4"), ("tangent_mass0", "<f4"), ("tangent_mass1", "<f4"),
                             ("normal_impulse", "<f4"), ("friction", "<f4")])
assert COMPONENT_DTYPE.itemsize == C.sizeof(Component) == 32
assert MOVING_DTYPE.itemsize == C.sizeof(MovingComponent) == 44
assert CONSTRAINT_DTYPE.itemsize == 96
# mgf_ray_hit: kind (HIT_*), index, part, inter = (p, t)
RAY_HIT_DTYPE = np.dtype([("kind", "<i4"), ("index", "<i4"), ("part", "<i4"), ("p", "<f4", 3), ("t", "<f4")])
assert RAY_HIT_DTYPE.itemsize == 28
# mgf_sweep_hit: kind (HIT_*), index, part, contact = (a, b, n, t)
SWEEP_HIT_DTYPE = np.dtype([("kind", "<i4"), ("index", "<i4"), ("part", "<i4"), ("a", "<f4", 3), ("b", "<f4", 3), ("n", "<f4", 3), ("t", "<f4")])
assert SWEEP_HIT_DTYPE.itemsize == 52
# mgf_body_contacts
BODY_CONTACTS_DTYPE = np.dtype([("n_contacts", "<i4"), ("n_terrain", "<i4"), ("impulse", "<f4", 3), ("normal_impulse", "<f4")])
assert BODY_CONTACTS_DTYPE.itemsize == 24
# what WorldBatch.get returns per record: mgf_velocity, mgf_rigid_body_info, and the force and torque rows
BODY_GET_DTYPE = np.dtype([("linear", "<f4", 3), ("angular", "<f4", 3), ("x", "<f4", 3), ("restitution", "<f4"), ("friction", "<f4"),
                           ("inv_mass", "<f4"), ("inv_moment", "<f4", 9), ("force", "<f4", 3), ("torque", "<f4", 3)])
HIT_NONE, HIT_BODY, HIT_TERRAIN, HIT_OBSTACLE = -1, 0, 1, 2
# mgf_batch_sensor: a ray fixed in the frame of body `body` of world `world`
SENSOR_DTYPE = np.dtype([("world", "<i4"), ("body", "<i4"), ("p", "<f4", 3), ("d", "<f4", 3), ("dt", "<f4"), ("flags", "<i4")])
# mgf_batch_camera: a pinhole camera fixed in the frame of body `body` of world `world`; r = (s, x, y, z)
CAMERA_DTYPE = np.dtype([("world", "<i4"), ("body", "<i4"), ("p", "<f4", 3), ("r", "<f4", 4), ("tan_x", "<f4"), ("tan_y", "<f4"), ("far", "<f4"),
                         ("width", "<i4"), ("height", "<i4"), ("flags", "<i4"), ("reserved", "<i4")])
assert CAMERA_DTYPE.itemsize == 64
# mgf_batch_zone: a box whose centre is fixed in the frame of body `body` of world `world` (body -1: in the world), half extents r
ZONE_DTYPE = np.dtype([("world", "<i4"), ("body", "<i4"), ("p", "<f4", 3), ("r", "<f4", 3), ("flags", "<i4"), ("reserved", "<i4")])
assert ZONE_DTYPE.itemsize == C.sizeof(BatchZone) == 40
BATCH_MAX_BODIES = 1024  # MGF_BATCH_MAX_BODIES
BATCH_MAX_WORLD_OBSTACLES = 64  # MGF_BATCH_MAX_WORLD_OBSTACLES
BATCH_DEV_SET_LAUNCHES = 3  # MGF_BATCH_DEV_SET_LAUNCHES
BATCH_DEV_QUERY_PLAN_LAUNCHES = 3  # MGF_BATCH_DEV_QUERY_PLAN_LAUNCHES
SENSOR_IGNORE_SELF = 1  # MGF_SENSOR_IGNORE_SELF
BATCH_SENSOR_LAUNCHES = 1  # MGF_BATCH_SENSOR_LAUNCHES
BATCH_CAMERA_LAUNCHES = 1  # MGF_BATCH_CAMERA_LAUNCHES
CAMERA_MAX_SIDE = 4096  # MGF_CAMERA_MAX_SIDE
BATCH_ZONE_LAUNCHES = 1  # MGF_BATCH_ZONE_LAUNCHES
BATCH_ZONE_NEAREST_MAX_K = 32  # MGF_BATCH_ZONE_NEAREST_MAX_K
BATCH_NEAREST_LAUNCHES = 1  # MGF_BATCH_NEAREST_LAUNCHES
# mgf_batch_touch: a contact sensor on body `body` of world `world`; other: a body of that world or TOUCH_STATIC / _ANY_BODY / _ANY
TOUCH_DTYPE = np.dtype([("world", "<i4"), ("body", "<i4"), ("other", "<i4"), ("flags", "<i4")])
# mgf_touch_report
TOUCH_REPORT_DTYPE = np.dtype([("n_contacts", "<i4"), ("partner", "<i4"), ("record", "<i4"), ("reserved0", "<i4"), ("impulse", "<f4", 3),
                               ("normal_impulse", "<f4"), ("push", "<f4", 3), ("strongest_impulse", "<f4"), ("arm", "<f4", 3), ("reserved1", "<f4")])
assert TOUCH_DTYPE.itemsize == 16 and TOUCH_REPORT_DTYPE.itemsize == 64
TOUCH_STATIC, TOUCH_ANY_BODY, TOUCH_ANY, TOUCH_NONE = -1, -2, -3, -4  # MGF_TOUCH_STATIC, _ANY_BODY, _ANY, _NONE
TOUCH_BODY_FRAME = 1  # MGF_TOUCH_BODY_FRAME
BATCH_TOUCH_LAUNCHES = 1  # MGF_BATCH_TOUCH_LAUNCHES
# mgf_batch_feeler: a sphere (tag 0) or capsule (tag 1) swept by delta, fixed in the frame of body `body` of world `world`
FEELER_DTYPE = np.dtype([("world", "<i4"), ("body", "<i4"), ("tag", "<i4"), ("flags", "<i4"), ("p", "<f4", 3), ("d", "<f4", 3), ("r", "<f4"),
                         ("delta", "<f4", 3), ("reserved", "<i4", 2)])
assert FEELER_DTYPE.itemsize == C.sizeof(BatchFeeler) == 64
FEELER_IGNORE_SELF, FEELER_WORLD_DELTA, FEELER_OWN_SHAPE = 1, 2, 4  # MGF_FEELER_IGNORE_SELF, _WORLD_DELTA, _OWN_SHAPE
BATCH_FEELER_LAUNCHES = 1  # MGF_BATCH_FEELER_LAUNCHES
# mgf_batch_actuator: a direction d and an arm p fixed in the frame of body `body` of world `world`, a gain and a clamp [lo, hi]
ACTUATOR_DTYPE = np.dtype([("world", "<i4"), ("body", "<i4"), ("flags", "<u4"), ("gain", "<f4"), ("p", "<f4", 3), ("lo", "<f4"),
                           ("d", "<f4", 3), ("hi", "<f4")])
assert ACTUATOR_DTYPE.itemsize == C.sizeof(BatchActuator) == 48
ACTUATOR_TORQUE, ACTUATOR_WORLD_DIR = 1, 2  # MGF_ACTUATOR_TORQUE, _WORLD_DIR
ACTUATE_IMPULSE, ACTUATE_FORCE = 0, 1  # MGF_ACTUATE_IMPULSE, _FORCE
BATCH_ACTUATOR_LAUNCHES = 1  # MGF_BATCH_ACTUATOR_LAUNCHES
BATCH_ROLLOUT_LAUNCHES_PER_TICK = 2  # MGF_BATCH_ROLLOUT_LAUNCHES_PER_TICK
# mgf_batch_spring: a spring-damper between the arm pa of body `body` and the arm pb of body `other` of world `world` (other = -1: pb
# is a point of the world), rest length, stiffness k, damping c and a clamp [lo, hi] of the scalar force
SPRING_DTYPE = np.dtype([("world", "<i4"), ("body", "<i4"), ("other", "<i4"), ("flags", "<u4"), ("pa", "<f4", 3), ("rest", "<f4"),
                         ("pb", "<f4", 3), ("k", "<f4"), ("c", "<f4"), ("lo", "<f4"), ("hi", "<f4"), ("pad", "<f4")])
assert SPRING_DTYPE.itemsize == C.sizeof(BatchSpring) == 64
BATCH_SPRING_LAUNCHES = 2  # MGF_BATCH_SPRING_LAUNCHES
BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK = 2  # MGF_BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK
# mgf_batch_joint: a ball joint between the anchor pa of body `body` and the anchor pb of body `other` of world `world` (other = -1: pb
# is a point of the world), beta the share of the position error removed per call
JOINT_DTYPE = np.dtype([("world", "<i4"), ("body", "<i4"), ("other", "<i4"), ("flags", "<u4"), ("pa", "<f4", 3), ("beta", "<f4"),
                        ("pb", "<f4", 3), ("pad", "<f4")])
assert JOINT_DTYPE.itemsize == C.sizeof(BatchJoint) == 48
BATCH_JOINT_LAUNCHES = 1  # MGF_BATCH_JOINT_LAUNCHES
BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK = 1  # MGF_BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK
BATCH_MAX_WORLD_JOINTS = 256  # MGF_BATCH_MAX_WORLD_JOINTS
# mgf_batch_hinge: a hinge between body `body` and body `other` of world `world` (other = -1: the world) - anchors pa, pb, unit axes ax, bx
# and unit zero-angle references ua, ub in each end's frame, beta the share of the position error removed per call, tmax the motor's
# largest torque, (cm, sm) and (ch, sh) the cosine and sine of the limit's middle and half range
HINGE_DTYPE = np.dtype([("world", "<i4"), ("body", "<i4"), ("other", "<i4"), ("flags", "<u4"), ("pa", "<f4", 3), ("beta", "<f4"),
                        ("pb", "<f4", 3), ("tmax", "<f4"), ("ax", "<f4", 3), ("cm", "<f4"), ("ua", "<f4", 3), ("sm", "<f4"),
                        ("bx", "<f4", 3), ("ch", "<f4"), ("ub", "<f4", 3), ("sh", "<f4")])
assert HINGE_DTYPE.itemsize == C.sizeof(BatchHinge) == 112
HINGE_LIMIT = 1  # MGF_HINGE_LIMIT
HINGE_MOTOR = 2  # MGF_HINGE_MOTOR
BATCH_HINGE_LAUNCHES = 1  # MGF_BATCH_HINGE_LAUNCHES
BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK = 1  # MGF_BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK
BATCH_MAX_WORLD_HINGES = 256  # MGF_BATCH_MAX_WORLD_HINGES
# mgf_batch_slider: a slider between body `body` and body `other` of world `world` (other = -1: the world) - anchors pa, pb, unit slide axes
# ax, bx and unit references ua, ub in each end's frame, beta the share of the position error removed per call, fmax the motor's largest
# force, [lo, hi] the travel range (with SLIDER_LOCK the travel held is lo)
SLIDER_DTYPE = np.dtype([("world", "<i4"), ("body", "<i4"), ("other", "<i4"), ("flags", "<u4"), ("pa", "<f4", 3), ("beta", "<f4"),
                         ("pb", "<f4", 3), ("fmax", "<f4"), ("ax", "<f4", 3), ("lo", "<f4"), ("ua", "<f4", 3), ("hi", "<f4"),
                         ("bx", "<f4", 3), ("pad0", "<f4"), ("ub", "<f4", 3), ("pad1", "<f4")])
assert SLIDER_DTYPE.itemsize == C.sizeof(BatchSlider) == 112
SLIDER_LIMIT = 1  # MGF_SLIDER_LIMIT
SLIDER_MOTOR = 2  # MGF_SLIDER_MOTOR
SLIDER_LOCK = 4  # MGF_SLIDER_LOCK
BATCH_SLIDER_LAUNCHES = 1  # MGF_BATCH_SLIDER_LAUNCHES
BATCH_ROLLOUT_SLIDER_LAUNCHES_PER_TICK = 1  # MGF_BATCH_ROLLOUT_SLIDER_LAUNCHES_PER_TICK
BATCH_MAX_WORLD_SLIDERS = 256  # MGF_BATCH_MAX_WORLD_SLIDERS
# mgf_hinge_reading: a hinge's encoder - cosine and sine of its angle, its rate, the side of its limit (+1, -1, 0: off), the anchors' gap
# in the world and the squared sine of the angle between the two axes; HINGE_TRACE_FULL_DTYPE: an entry of the readings table in the full
# format - the reading and the eight impulse words of the tick's hinge solve (am / dt: the motor's torque)
HINGE_READING_DTYPE = np.dtype([("c", "<f4"), ("sn", "<f4"), ("rate", "<f4"), ("side", "<f4"), ("gap", "<f4", 3), ("tilt2", "<f4")])
HINGE_TRACE_FULL_DTYPE = np.dtype([("c", "<f4"), ("sn", "<f4"), ("rate", "<f4"), ("side", "<f4"), ("gap", "<f4", 3), ("tilt2", "<f4"),
                                   ("acc", "<f4", 3), ("a1", "<f4"), ("a2", "<f4"), ("al", "<f4"), ("am", "<f4"), ("pad", "<f4")])
assert HINGE_READING_DTYPE.itemsize == 32 and HINGE_TRACE_FULL_DTYPE.itemsize == 64
HINGE_TRACE_READING, HINGE_TRACE_FULL = 0, 1  # MGF_HINGE_TRACE_READING, _FULL
BATCH_HINGE_READ_LAUNCHES = 1  # MGF_BATCH_HINGE_READ_LAUNCHES
BATCH_ROLLOUT_HINGE_READ_LAUNCHES_PER_TICK = 1  # MGF_BATCH_ROLLOUT_HINGE_READ_LAUNCHES_PER_TICK
# mgf_slider_reading: a slider's encoder - its travel along the axis, its rate as the next solve's axis rows see it, the side of its
# limit (+1, -1; 2: locked; 0: off), the far anchor's distance from the axis along the two references and the frames' error;
# SLIDER_TRACE_FULL_DTYPE: an entry of the readings table in the full format - the reading and the eight impulse words of the tick's
# slider solve (am / dt: the motor's force)
SLIDER_READING_DTYPE = np.dtype([("d", "<f4"), ("rate", "<f4"), ("side", "<f4"), ("off", "<f4", 2), ("e", "<f4", 3)])
SLIDER_TRACE_FULL_DTYPE = np.dtype([("d", "<f4"), ("rate", "<f4"), ("side", "<f4"), ("off", "<f4", 2), ("e", "<f4", 3),
                                    ("p1", "<f4"), ("p2", "<f4"), ("al", "<f4"), ("am", "<f4"), ("aw", "<f4", 3), ("pad", "<f4")])
assert SLIDER_READING_DTYPE.itemsize == 32 and SLIDER_TRACE_FULL_DTYPE.itemsize == 64
SLIDER_TRACE_READING, SLIDER_TRACE_FULL = 0, 1  # MGF_SLIDER_TRACE_READING, _FULL
BATCH_SLIDER_READ_LAUNCHES = 1  # MGF_BATCH_SLIDER_READ_LAUNCHES
BATCH_ROLLOUT_SLIDER_READ_LAUNCHES_PER_TICK = 1  # MGF_BATCH_ROLLOUT_SLIDER_READ_LAUNCHES_PER_TICK
# what WorldBatch's encoder helpers take of a kind: its word in the methods and the symbols, the reading's and the full entry's dtype, the two formats
_HINGE_ENC = ("hinge", HINGE_READING_DTYPE, HINGE_TRACE_FULL_DTYPE, HINGE_TRACE_READING, HINGE_TRACE_FULL)
_SLIDER_ENC = ("slider", SLIDER_READING_DTYPE, SLIDER_TRACE_FULL_DTYPE, SLIDER_TRACE_READING, SLIDER_TRACE_FULL)
# mgf_touch_short: an entry of a rollout's touch rows in the short format - four words of mgf_touch_report
TOUCH_SHORT_DTYPE = np.dtype([("n_contacts", "<i4"), ("partner", "<i4"), ("normal_impulse", "<f4"), ("strongest_impulse", "<f4")])
assert TOUCH_SHORT_DTYPE.itemsize == 16
ROLLOUT_TOUCH_FULL, ROLLOUT_TOUCH_SHORT = 0, 1  # MGF_ROLLOUT_TOUCH_FULL, _SHORT
BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK = 1  # MGF_BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK
ROLLOUT_SENSOR_HIT, ROLLOUT_SENSOR_DEPTH = 0, 1  # MGF_ROLLOUT_SENSOR_HIT, _DEPTH
BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK = 2  # MGF_BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK


class ROLLOUT_TRACES(C.Structure):
    """mgf_rollout_traces: the traces of mgf_batch_rollout_observe / _observe_dev, 64 bytes"""
    _fields_ = [("touch", C.c_void_p), ("n_touch", C.c_int64), ("sensor", C.c_void_p), ("n_sensor", C.c_int64),
                ("touch_format", C.c_int32), ("sensor_format", C.c_int32), ("sensor_mask", C.c_int32), ("reserved", C.c_int32 * 5)]


assert C.sizeof(ROLLOUT_TRACES) == 64
QUERY_BODIES, QUERY_TERRAIN, QUERY_OBSTACLES, QUERY_ALL = 1, 2, 4, 7

# every symbol include/mgf_hip.h declares (tests check the library exports all of them)
SYMBOLS = [
    "mgf_ctx_create", "mgf_ctx_destroy", "mgf_ctx_set_stream", "mgf_last_error", "mgf_default_params", "mgf_version", "mgf_exclusive_scan_u32",
    "mgf_contacts", "mgf_contacts_batch", "mgf_tri_reject_batch", "mgf_local_contacts_pair", "mgf_ray_capsule", "mgf_inertia_tensor",
    "mgf_mesh_new", "mgf_mesh_free", "mgf_mesh_push_vert", "mgf_mesh_push_face", "mgf_mesh_set_pos", "mgf_mesh_build",
    "mgf_local_contacts_mesh",
    "mgf_bvh_new", "mgf_bvh_with_capacity", "mgf_bvh_free", "mgf_bvh_empty", "mgf_bvh_clear", "mgf_bvh_insert",
    "mgf_bvh_remove", "mgf_bvh_root", "mgf_bvh_get_leaf", "mgf_bvh_bounds", "mgf_bvh_query", "mgf_bvh_query_many",
    "mgf_bvh_raytrace", "mgf_bvh_raytrace_many", "mgf_intersections_batch",
    "mgf_compound_new", "mgf_compound_free", "mgf_compound_set_pose", "mgf_compound_bounds", "mgf_compound_contacts_many",
    "mgf_compound_intersections",
    "mgf_bvh_to_json", "mgf_bvh_from_json", "mgf_mesh_to_json", "mgf_mesh_from_json", "mgf_manifolds_from_contacts",
    "mgf_world_new", "mgf_world_free", "mgf_world_set_terrain", "mgf_world_add_bodies", "mgf_world_add_compound_bodies", "mgf_world_len",
    "mgf_world_step", "mgf_world_step_many", "mgf_world_build_constraints", "mgf_world_solve", "mgf_world_complete_motion",
    "mgf_world_integrate", "mgf_world_get", "mgf_world_set", "mgf_world_read_state", "mgf_world_write_state",
    "mgf_world_read_colliders", "mgf_world_raycast_many", "mgf_world_sweep_many", "mgf_world_overlap_aabb_many", "mgf_world_read_constraints", "mgf_world_set_constraints", "mgf_world_set_option",
    "mgf_world_device_ptr",
    "mgf_world_release_device_ptrs",
    "mgf_world_begin_tick", "mgf_world_collide", "mgf_world_select_boundary", "mgf_world_export_bodies",
    "mgf_world_import_ghosts", "mgf_world_export_velocities", "mgf_world_import_ghost_velocities", "mgf_world_ghost_len",
    "mgf_world_select_tile", "mgf_world_export_migrants", "mgf_world_remove_bodies", "mgf_world_import_migrants",
    "mgf_world_set_tags", "mgf_world_read_tags",
    "mgf_world_solve_enqueue", "mgf_world_finish", "mgf_world_counter",
    "mgf_constraints_new", "mgf_solver_new", "mgf_solver_free", "mgf_solver_add_constraint", "mgf_solver_add_constraints",
    "mgf_solver_len", "mgf_solver_clear", "mgf_solver_read_constraints", "mgf_solver_solve", "mgf_world_clone",
    "mgf_geom_to_json", "mgf_geom_from_json",
    "mgf_tiles_create", "mgf_tiles_free", "mgf_rccl_unique_id", "mgf_rccl_allow_override", "mgf_tiles_connect", "mgf_tiles_preflight", "mgf_tiles_step",
    "mgf_tiles_migrated", "mgf_tiles_set_option", "mgf_world_add_obstacle", "mgf_tiles_counter",
    "mgf_batch_new", "mgf_batch_free", "mgf_batch_set_terrain", "mgf_batch_add_terrain", "mgf_batch_set_world_terrain",
    "mgf_batch_terrain_count", "mgf_batch_add_bodies", "mgf_batch_add_compound_bodies", "mgf_batch_len", "mgf_batch_step",
    "mgf_batch_read_state", "mgf_batch_write_state", "mgf_batch_read_constraints", "mgf_batch_counter", "mgf_batch_set_option",
    "mgf_batch_read_colliders", "mgf_batch_raycast_many", "mgf_batch_sweep_many",
    "mgf_batch_read_body_contacts", "mgf_batch_overlap_aabb_many",
    "mgf_batch_get_many", "mgf_batch_set_many", "mgf_batch_set_forces", "mgf_batch_apply_impulses", "mgf_batch_copy_worlds",
    "mgf_batch_add_obstacle", "mgf_batch_set_world_obstacles", "mgf_batch_obstacle_count", "mgf_batch_world_obstacle_count",
    "mgf_ctx_synchronize", "mgf_batch_gather_state_dev", "mgf_batch_set_many_dev", "mgf_batch_set_forces_dev", "mgf_batch_apply_impulses_dev",
    "mgf_batch_read_body_contacts_dev", "mgf_batch_copy_worlds_where", "mgf_batch_raycast_many_dev", "mgf_batch_sweep_many_dev",
    "mgf_batch_set_sensors", "mgf_batch_sensor_count", "mgf_batch_cast_sensors", "mgf_batch_cast_sensors_dev",
    "mgf_batch_set_cameras", "mgf_batch_camera_count", "mgf_batch_camera_pixels", "mgf_batch_cast_cameras", "mgf_batch_cast_cameras_dev",
    "mgf_batch_set_zones", "mgf_batch_zone_count", "mgf_batch_read_zones", "mgf_batch_read_zones_dev", "mgf_batch_overlap_first_dev",
    "mgf_batch_read_zones_nearest", "mgf_batch_read_zones_nearest_dev", "mgf_batch_overlap_nearest_dev",
    "mgf_batch_set_touches", "mgf_batch_touch_count", "mgf_batch_read_touches", "mgf_batch_read_touches_dev",
    "mgf_batch_set_feelers", "mgf_batch_feeler_count", "mgf_batch_cast_feelers", "mgf_batch_cast_feelers_dev",
    "mgf_batch_set_actuators", "mgf_batch_actuator_count", "mgf_batch_actuate", "mgf_batch_actuate_dev",
    "mgf_batch_rollout", "mgf_batch_rollout_dev", "mgf_batch_rollout_touches", "mgf_batch_rollout_touches_dev",
    "mgf_batch_rollout_observe", "mgf_batch_rollout_observe_dev",
    "mgf_batch_set_springs", "mgf_batch_spring_count", "mgf_batch_apply_springs", "mgf_batch_apply_springs_dev",
    "mgf_batch_set_joints", "mgf_batch_joint_count", "mgf_batch_solve_joints", "mgf_batch_solve_joints_dev",
    "mgf_batch_set_hinges", "mgf_batch_hinge_count", "mgf_batch_set_hinge_targets", "mgf_batch_set_hinge_targets_dev",
    "mgf_batch_solve_hinges", "mgf_batch_solve_hinges_dev",
    "mgf_batch_read_hinges", "mgf_batch_read_hinges_dev", "mgf_batch_set_hinge_trace", "mgf_batch_hinge_trace_rows",
    "mgf_batch_get_hinge_trace", "mgf_batch_get_hinge_trace_dev",
    "mgf_batch_read_sliders", "mgf_batch_read_sliders_dev", "mgf_batch_set_slider_trace", "mgf_batch_slider_trace_rows",
    "mgf_batch_get_slider_trace", "mgf_batch_get_slider_trace_dev",
    "mgf_batch_set_sliders", "mgf_batch_slider_count", "mgf_batch_set_slider_targets", "mgf_batch_set_slider_targets_dev",
    "mgf_batch_solve_sliders", "mgf_batch_solve_sliders_dev",
]

_lib = None
HIT_FN = C.CFUNCTYPE(None, C.POINTER(C.c_uint64), C.c_void_p)
RAY_FN = C.CFUNCTYPE(None, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p)


def load_library():
    """dlopen mgf_amd/libmgf_hip.so.  Raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise MgfError(ERR_HIP, f"{path} is missing: build it with `python -m mgf_amd.build` (hipcc, gfx950). "
                                "mgf_amd has no CPU fallback.")
    L = C.CDLL(path)
    P, vp, i32, i64, u64, f32 = C.POINTER, C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float
    sig = {
        "mgf_ctx_create": (i32, [C.c_int, P(vp)]),
        "mgf_ctx_destroy": (None, [vp]),
        "mgf_ctx_set_stream": (i32, [vp, vp]),
        "mgf_last_error": (C.c_char_p, []),
        "mgf_default_params": (Params, []),
        "mgf_version": (C.c_char_p, []),
        "mgf_exclusive_scan_u32": (i32, [vp, vp, i64, vp]),
        "mgf_contacts": (i32, [vp, P(Shape), P(Vec3), P(Shape), P(Vec3), P(Contact), i32, P(i32)]),
        "mgf_contacts_batch": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, vp]),
        "mgf_tri_reject_batch": (i32, [vp, i64, vp, vp, vp, vp]),
        "mgf_local_contacts_pair": (i32, [vp, P(MovingComponent), P(MovingComponent), P(LocalContact), i32, P(i32)]),
        "mgf_ray_capsule": (i32, [vp, P(Vec3), P(Vec3), P(Shape), P(Vec3), P(f32), P(i32)]),
        "mgf_inertia_tensor": (i32, [P(Component), f32, P(f32)]),
        "mgf_mesh_new": (i32, [vp, P(vp)]),
        "mgf_mesh_free": (None, [vp]),
        "mgf_mesh_push_vert": (i32, [vp, Vec3, P(u64)]),
        "mgf_mesh_push_face": (i32, [vp, u64, u64, u64, P(u64)]),
        "mgf_mesh_set_pos": (i32, [vp, Vec3]),
        "mgf_mesh_build": (i32, [vp, vp, i64, vp, i64]),
        "mgf_mesh_bvh_view": (vp, [vp]),
        "mgf_local_contacts_mesh": (i32, [vp, P(MovingComponent), vp, P(LocalContact), i32, P(i32)]),
        "mgf_bvh_new": (i32, [vp, P(vp)]),
        "mgf_bvh_with_capacity": (i32, [vp, u64, P(vp)]),
        "mgf_bvh_free": (None, [vp]),
        "mgf_bvh_empty": (i32, [vp]),
        "mgf_bvh_clear": (i32, [vp]),
        "mgf_bvh_insert": (i32, [vp, P(Aabb), u64, P(u64)]),
        "mgf_bvh_remove": (i32, [vp, u64]),
        "mgf_bvh_root": (i32, [vp, P(u64)]),
        "mgf_bvh_get_leaf": (i32, [vp, u64, P(u64)]),
        "mgf_bvh_bounds": (i32, [vp, u64, P(Aabb)]),
        "mgf_bvh_query": (i32, [vp, P(Aabb), HIT_FN, vp]),
        "mgf_bvh_query_many": (i32, [vp, vp, i64, vp, vp, i64, P(i64)]),
        "mgf_bvh_raytrace": (i32, [vp, vp, RAY_FN, vp]),
        "mgf_bvh_raytrace_many": (i32, [vp, vp, i64, vp, vp, vp, i64, P(i64)]),
        "mgf_intersections_batch": (i32, [vp, i64, vp, vp, vp, vp, vp]),
        "mgf_compound_new": (i32, [vp, vp, i64, P(vp)]),
        "mgf_compound_free": (None, [vp]),
        "mgf_compound_set_pose": (i32, [vp, Vec3, Quat]),
        "mgf_compound_bounds": (i32, [vp, P(Aabb)]),
        "mgf_compound_contacts_many": (i32, [vp, vp, i64, vp, vp, i64, P(i64)]),
        "mgf_compound_intersections": (i32, [vp, vp, i64, vp, vp]),
        "mgf_bvh_to_json": (i32, [vp, vp, i64, P(i64)]),
        "mgf_bvh_from_json": (i32, [vp, C.c_char_p, i64, P(vp)]),
        "mgf_mesh_to_json": (i32, [vp, vp, i64, P(i64)]),
        "mgf_mesh_from_json": (i32, [vp, C.c_char_p, i64, P(vp)]),
        "mgf_manifolds_from_contacts": (i32, [vp, vp, i64, vp, vp, vp]),
        "mgf_bvh_dump": (i64, [vp, vp, vp, i64]),
        "mgf_world_new": (i32, [vp, P(Params), P(vp)]),
        "mgf_world_free": (None, [vp]),
        "mgf_world_set_terrain": (i32, [vp, vp]),
        "mgf_world_add_bodies": (i32, [vp, vp, i64, vp, vp, vp, vp, P(u64)]),
        "mgf_world_add_compound_bodies": (i32, [vp, vp, vp, vp, i64, vp, vp, vp, P(u64)]),
        "mgf_world_len": (i64, [vp]),
        "mgf_world_step": (i32, [vp, f32, i32, P(StepStats)]),
        "mgf_world_step_many": (i32, [vp, f32, i32, i64, vp]),
        "mgf_world_build_constraints": (i32, [vp, f32, P(StepStats)]),
        "mgf_world_solve": (i32, [vp, i32, P(StepStats)]),
        "mgf_world_complete_motion": (i32, [vp]),
        "mgf_world_integrate": (i32, [vp, f32]),
        "mgf_world_get": (i32, [vp, P(BodyRef), P(Velocity), P(RigidBodyInfo)]),
        "mgf_world_set": (i32, [vp, P(BodyRef), P(Velocity)]),
        "mgf_world_read_state": (i32, [vp, vp, vp, vp, vp, vp, i64]),
        "mgf_world_write_state": (i32, [vp, vp, vp, vp, vp, vp, i64]),
        "mgf_world_read_colliders": (i32, [vp, vp, i64]),
        "mgf_world_raycast_many": (i32, [vp, vp, i64, vp, C.c_int32, vp]),
        "mgf_world_sweep_many": (i32, [vp, vp, i64, vp, C.c_int32, vp]),
        "mgf_world_overlap_aabb_many": (i32, [vp, vp, i64, vp, vp, i64, P(i64)]),
        "mgf_world_read_constraints": (i32, [vp, vp, i64, P(i64)]),
        "mgf_world_set_constraints": (i32, [vp, vp, i64]),
        "mgf_world_set_option": (i32, [vp, C.c_char_p, i64]),
        "mgf_world_device_ptr": (i32, [vp, C.c_char_p, P(vp), P(i64)]),
        "mgf_world_release_device_ptrs": (i32, [vp]),
        "mgf_world_begin_tick": (i32, [vp, f32]),
        "mgf_world_collide": (i32, [vp, f32, P(StepStats)]),
        "mgf_world_select_boundary": (i32, [vp, f32, f32, vp, vp, i64, P(i64), P(i64)]),
        "mgf_world_export_bodies": (i32, [vp, vp, i64, vp]),
        "mgf_world_import_ghosts": (i32, [vp, vp, i64]),
        "mgf_world_export_velocities": (i32, [vp, vp, i64, vp]),
        "mgf_world_import_ghost_velocities": (i32, [vp, vp, i64]),
        "mgf_world_ghost_len": (i64, [vp]),
        "mgf_world_select_tile": (i32, [vp, f32, f32, f32, f32, vp, vp, vp, i64, P(i64)]),
        "mgf_world_export_migrants": (i32, [vp, vp, i64, vp]),
        "mgf_world_remove_bodies": (i32, [vp, vp, i64]),
        "mgf_world_import_migrants": (i32, [vp, vp, i64]),
        "mgf_world_set_tags": (i32, [vp, vp, i64]),
        "mgf_world_read_tags": (i32, [vp, vp, i64]),
        "mgf_world_solve_enqueue": (i32, [vp, i32]),
        "mgf_world_finish": (i32, [vp, P(StepStats)]),
        "mgf_world_counter": (i32, [vp, C.c_char_p, P(i64)]),
        "mgf_constraints_new": (i32, [vp, vp, vp, vp, i64, f32, vp, i64, P(i64)]),
        "mgf_solver_new": (i32, [P(vp)]),
        "mgf_solver_free": (None, [vp]),
        "mgf_solver_add_constraint": (i32, [vp, vp]),
        "mgf_solver_add_constraints": (i32, [vp, vp, i64]),
        "mgf_solver_len": (i64, [vp]),
        "mgf_solver_clear": (i32, [vp]),
        "mgf_solver_read_constraints": (i32, [vp, vp, i64, P(i64)]),
        "mgf_solver_solve": (i32, [vp, vp, i32, P(StepStats)]),
        "mgf_world_clone": (i32, [vp, P(vp)]),
        "mgf_geom_to_json": (i32, [P(Shape), P(Vec3), vp, i64, P(i64)]),
        "mgf_geom_from_json": (i32, [i32, C.c_char_p, i64, P(Shape), P(Vec3)]),
        "mgf_tiles_create": (i32, [vp, i32, vp, vp, vp, i32, i32, f32, i32, i32, P(vp)]),
        "mgf_tiles_free": (None, [vp]),
        "mgf_rccl_unique_id": (i32, [vp]),
        "mgf_rccl_allow_override": (i32, [C.c_int32]),
        "mgf_tiles_connect": (i32, [vp, vp, i32, i32]),
        "mgf_tiles_preflight": (i32, [vp, P(i32)]),
        "mgf_tiles_step": (i32, [vp, f32, i32, vp]),
        "mgf_tiles_migrated": (i64, [vp, i32, i32]),
        "mgf_tiles_counter": (i64, [vp, C.c_char_p]),
        "mgf_tiles_set_option": (i32, [vp, C.c_char_p, i64]),
        "mgf_world_add_obstacle": (i32, [vp, vp]),
        "mgf_batch_new": (i32, [vp, P(Params), i64, P(vp)]),
        "mgf_batch_free": (None, [vp]),
        "mgf_batch_set_terrain": (i32, [vp, vp]),
        "mgf_batch_add_terrain": (i32, [vp, vp, P(i32)]),
        "mgf_batch_set_world_terrain": (i32, [vp, vp, vp, vp, i64]),
        "mgf_batch_terrain_count": (i64, [vp]),
        "mgf_batch_add_bodies": (i32, [vp, i64, vp, i64, vp, vp, vp, vp, P(u64)]),
        "mgf_batch_add_compound_bodies": (i32, [vp, i64, vp, vp, vp, i64, vp, vp, vp, P(u64)]),
        "mgf_batch_len": (i64, [vp, i64]),
        "mgf_batch_step": (i32, [vp, f32, i32, i64, vp]),
        "mgf_batch_read_state": (i32, [vp, i64, vp, vp, vp, vp, vp, i64]),
        "mgf_batch_write_state": (i32, [vp, i64, vp, vp, vp, vp, vp, i64]),
        "mgf_batch_read_constraints": (i32, [vp, i64, vp, i64, P(i64)]),
        "mgf_batch_counter": (i32, [vp, C.c_char_p, P(i64)]),
        "mgf_batch_set_option": (i32, [vp, C.c_char_p, i64]),
        "mgf_batch_read_colliders": (i32, [vp, i64, vp, i64]),
        "mgf_batch_raycast_many": (i32, [vp, vp, vp, i64, vp, i32, vp]),
        "mgf_batch_sweep_many": (i32, [vp, vp, vp, i64, vp, i32, vp]),
        "mgf_batch_read_body_contacts": (i32, [vp, i64, vp, i64]),
        "mgf_batch_overlap_aabb_many": (i32, [vp, vp, vp, i64, vp, vp, i64, P(i64)]),
        "mgf_batch_get_many": (i32, [vp, vp, vp, i64, vp, vp, vp, vp]),
        "mgf_batch_set_many": (i32, [vp, vp, vp, i64, vp]),
        "mgf_batch_set_forces": (i32, [vp, vp, vp, i64, vp, vp]),
        "mgf_batch_apply_impulses": (i32, [vp, vp, vp, i64, vp, vp]),
        "mgf_batch_copy_worlds": (i32, [vp, vp, vp, vp, i64]),
        "mgf_batch_add_obstacle": (i32, [vp, vp, P(i32)]),
        "mgf_batch_set_world_obstacles": (i32, [vp, vp, vp, vp, vp, i64]),
        "mgf_batch_obstacle_count": (i64, [vp]),
        "mgf_batch_world_obstacle_count": (i64, [vp, i64]),
        "mgf_ctx_synchronize": (i32, [vp]),
        "mgf_batch_gather_state_dev": (i32, [vp, vp, i64, vp, vp, vp, vp, vp, vp]),
        "mgf_batch_set_many_dev": (i32, [vp, vp, i64, vp, vp]),
        "mgf_batch_set_forces_dev": (i32, [vp, vp, i64, vp, vp]),
        "mgf_batch_apply_impulses_dev": (i32, [vp, vp, i64, vp, vp]),
        "mgf_batch_read_body_contacts_dev": (i32, [vp, i64, vp, i64]),
        "mgf_batch_raycast_many_dev": (i32, [vp, vp, vp, i64, vp, i32, vp]),
        "mgf_batch_sweep_many_dev": (i32, [vp, vp, vp, i64, vp, i32, vp]),
        "mgf_batch_copy_worlds_where": (i32, [vp, vp, vp, vp, i64, vp]),
        "mgf_batch_set_sensors": (i32, [vp, vp, i64]),
        "mgf_batch_sensor_count": (i64, [vp]),
        "mgf_batch_cast_sensors": (i32, [vp, i32, vp, vp, i64]),
        "mgf_batch_cast_sensors_dev": (i32, [vp, i32, vp, vp, i64]),
        "mgf_batch_set_zones": (i32, [vp, vp, i64]),
        "mgf_batch_zone_count": (i64, [vp]),
        "mgf_batch_read_zones": (i32, [vp, i32, vp, vp, i64]),
        "mgf_batch_read_zones_dev": (i32, [vp, i32, vp, vp, i64]),
        "mgf_batch_overlap_first_dev": (i32, [vp, vp, i64, vp, i32, vp]),
        "mgf_batch_read_zones_nearest": (i32, [vp, i32, vp, vp, vp, i64]),
        "mgf_batch_read_zones_nearest_dev": (i32, [vp, i32, vp, vp, vp, i64]),
        "mgf_batch_overlap_nearest_dev": (i32, [vp, vp, i64, vp, i32, vp, vp]),
        "mgf_batch_set_touches": (i32, [vp, vp, i64]),
        "mgf_batch_touch_count": (i64, [vp]),
        "mgf_batch_read_touches": (i32, [vp, vp, i64]),
        "mgf_batch_read_touches_dev": (i32, [vp, vp, i64]),
        "mgf_batch_set_feelers": (i32, [vp, vp, i64]),
        "mgf_batch_feeler_count": (i64, [vp]),
        "mgf_batch_cast_feelers": (i32, [vp, i32, vp, vp, i64]),
        "mgf_batch_cast_feelers_dev": (i32, [vp, i32, vp, vp, i64]),
        "mgf_batch_set_actuators": (i32, [vp, vp, i64]),
        "mgf_batch_actuator_count": (i64, [vp]),
        "mgf_batch_actuate": (i32, [vp, vp, i64, i32, vp]),
        "mgf_batch_actuate_dev": (i32, [vp, vp, i64, i32, vp]),
        "mgf_batch_rollout": (i32, [vp, f32, i32, i64, vp, i64, i32, vp, i64, vp, vp, vp, vp, vp]),
        "mgf_batch_rollout_dev": (i32, [vp, f32, i32, i64, vp, i64, i32, vp, i64, vp, vp, vp, vp, vp]),
        "mgf_batch_rollout_touches": (i32, [vp, f32, i32, i64, vp, i64, i32, vp, i64, vp, vp, vp, vp, vp, i64, i32, vp]),
        "mgf_batch_rollout_touches_dev": (i32, [vp, f32, i32, i64, vp, i64, i32, vp, i64, vp, vp, vp, vp, vp, i64, i32, vp]),
        "mgf_batch_rollout_observe": (i32, [vp, f32, i32, i64, vp, i64, i32, vp, i64, vp, vp, vp, vp, C.POINTER(ROLLOUT_TRACES), vp]),
        "mgf_batch_rollout_observe_dev": (i32, [vp, f32, i32, i64, vp, i64, i32, vp, i64, vp, vp, vp, vp, C.POINTER(ROLLOUT_TRACES), vp]),
        "mgf_batch_set_springs": (i32, [vp, vp, i64]),
        "mgf_batch_spring_count": (i64, [vp]),
        "mgf_batch_apply_springs": (i32, [vp, f32, vp]),
        "mgf_batch_apply_springs_dev": (i32, [vp, f32, vp]),
        "mgf_batch_set_joints": (i32, [vp, vp, i64]),
        "mgf_batch_joint_count": (i64, [vp]),
        "mgf_batch_solve_joints": (i32, [vp, f32, i32, vp]),
        "mgf_batch_solve_joints_dev": (i32, [vp, f32, i32, vp]),
        "mgf_batch_set_hinges": (i32, [vp, vp, i64]),
        "mgf_batch_hinge_count": (i64, [vp]),
        "mgf_batch_set_hinge_targets": (i32, [vp, vp, i64]),
        "mgf_batch_set_hinge_targets_dev": (i32, [vp, vp, i64]),
        "mgf_batch_solve_hinges": (i32, [vp, f32, i32, i64, vp]),
        "mgf_batch_solve_hinges_dev": (i32, [vp, f32, i32, i64, vp]),
        "mgf_batch_read_hinges": (i32, [vp, vp]),
        "mgf_batch_read_hinges_dev": (i32, [vp, vp]),
        "mgf_batch_set_hinge_trace": (i32, [vp, i64, i32]),
        "mgf_batch_hinge_trace_rows": (i64, [vp]),
        "mgf_batch_get_hinge_trace": (i32, [vp, vp, i64, i64]),
        "mgf_batch_get_hinge_trace_dev": (i32, [vp, vp, i64, i64]),
        "mgf_batch_read_sliders": (i32, [vp, vp]),
        "mgf_batch_read_sliders_dev": (i32, [vp, vp]),
        "mgf_batch_set_slider_trace": (i32, [vp, i64, i32]),
        "mgf_batch_slider_trace_rows": (i64, [vp]),
        "mgf_batch_get_slider_trace": (i32, [vp, vp, i64, i64]),
        "mgf_batch_get_slider_trace_dev": (i32, [vp, vp, i64, i64]),
        "mgf_batch_set_sliders": (i32, [vp, vp, i64]),
        "mgf_batch_slider_count": (i64, [vp]),
        "mgf_batch_set_slider_targets": (i32, [vp, vp, i64]),
        "mgf_batch_set_slider_targets_dev": (i32, [vp, vp, i64]),
        "mgf_batch_solve_sliders": (i32, [vp, f32, i32, i64, vp]),
        "mgf_batch_solve_sliders_dev": (i32, [vp, f32, i32, i64, vp]),
        "mgf_batch_set_cameras": (i32, [vp, vp, i64]),
        "mgf_batch_camera_count": (i64, [vp]),
        "mgf_batch_camera_pixels": (i64, [vp]),
        "mgf_batch_cast_cameras": (i32, [vp, i32, vp, vp, vp, i64]),
        "mgf_batch_cast_cameras_dev": (i32, [vp, i32, vp, vp, vp, i64]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _check(status):
    if status != 0:
        raise MgfError(status, load_library().mgf_last_error().decode(errors="replace"))


def _v3(v):
    return Vec3(float(v[0]), float(v[1]), float(v[2]))


def default_params():
    return load_library().mgf_default_params()


def inertia_tensor(tag, p, d, r, mass):
    """Inertia::tensor (physics.rs:26-93): column-major 3x3 as a flat list of 9."""
    out = (C.c_float * 9)()
    _check(load_library().mgf_inertia_tensor(C.byref(Component(tag, _v3(p), _v3(d), float(r))), float(mass), out))
    return [out[i] for i in range(9)]


class Context:
    """One per GPU (device + HIP stream).  Raises MgfError(HIP) when no GPU is present."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        self._children = weakref.WeakSet()
        _check(load_library().mgf_ctx_create(int(device), C.byref(self._h)))

    def _adopt(self, obj):
        self._children.add(obj)

    def exclusive_scan(self, counts):
        """out[i] = sum(counts[:i]) on the device (the tick's own scan primitive)."""
        a = np.ascontiguousarray(counts, np.uint32)
        out = np.zeros(len(a), np.uint32)
        _check(load_library().mgf_exclusive_scan_u32(self._h, a.ctypes.data, len(a), out.ctypes.data))
        return out

    def set_stream(self, hip_stream):
        """Enqueue this context's work on a caller-owned hipStream_t (an int handle, e.g. torch's cuda_stream)."""
        _check(load_library().mgf_ctx_set_stream(self._h, C.c_void_p(int(hip_stream))))

    def synchronize(self):
        """Wait for this context's stream (mgf_ctx_synchronize) - and for nothing else on the device"""
        _check(load_library().mgf_ctx_synchronize(self._h))

    def close(self):
        """Destroy the context; handles created from it are released first.  (A handle that outlives it all the same - an interpreter's
        finalisation clears the weak references before it runs the finalisers, in any order - keeps the C side's struct and streams alive until
        it is freed: mgf_ctx_destroy only drops the creator's reference.)"""
        if getattr(self, "_h", None):
            for child in list(self._children):
                child.__del__()
            load_library().mgf_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _shape(d):
    s = Shape()
    k = d["kind"]
    if k == "sphere":
        s.kind, vals = SPHERE, list(d["c"]) + [d["r"]]
    elif k == "capsule":
        s.kind, vals = CAPSULE, list(d["a"]) + list(d["d"]) + [d["r"]]
    elif k == "triangle":
        s.kind, vals = TRIANGLE, list(d["a"]) + list(d["b"]) + list(d["c"])
    elif k == "plane":
        s.kind, vals = PLANE, list(d["n"]) + [d["d"]]
    elif k == "rectangle":
        s.kind, vals = RECTANGLE, list(d["c"]) + list(d["u0"]) + list(d["u1"]) + list(d["e"])
    elif k == "ray":
        s.kind, vals = RAY, list(d["p"]) + list(d["d"])
    elif k == "segment":
        s.kind, vals = SEGMENT, list(d["a"]) + list(d["b"])
    elif k == "aabb":
        s.kind, vals = AABB, list(d["c"]) + list(d["r"])
    else:
        raise ValueError(k)
    for i, x in enumerate(vals):
        s.v[i] = float(x)
    return s


_GEOM_FIELDS = {"sphere": (SPHERE, [("c", 3), ("r", 1)]), "capsule": (CAPSULE, [("a", 3), ("d", 3), ("r", 1)]),
                "triangle": (TRIANGLE, [("a", 3), ("b", 3), ("c", 3)]), "plane": (PLANE, [("n", 3), ("d", 1)]),
                "rectangle": (RECTANGLE, [("c", 3), ("u0", 3), ("u1", 3), ("e", 2)]), "ray": (RAY, [("p", 3), ("d", 3)]),
                "segment": (SEGMENT, [("a", 3), ("b", 3)]), "aabb": (AABB, [("c", 3), ("r", 3)])}


def geom_to_json(shape, moving=None):
    """serde_json text of a geom.rs struct given as a shape dict (kind + fields); moving = the Vector3 of Moving<T>."""
    n = C.c_int64()
    sh = _shape(shape)
    mv = C.byref(_v3(moving)) if moving is not None else None
    st = load_library().mgf_geom_to_json(C.byref(sh), mv, None, 0, C.byref(n))
    if st != ERR_CAPACITY:
        _check(st)
    buf = C.create_string_buffer(n.value + 1)
    _check(load_library().mgf_geom_to_json(C.byref(sh), mv, buf, n.value + 1, C.byref(n)))
    return buf.value.decode()


def geom_from_json(kind, text, moving=False):
    """the shape dict of `kind` ("sphere", "capsule", ...) read from serde_json text; moving=True reads Moving<T> and returns
    (shape, velocity)."""
    code, fields = _GEOM_FIELDS[kind]
    raw = text.encode()
    out, vel = Shape(), Vec3()
    _check(load_library().mgf_geom_from_json(code, raw, len(raw), C.byref(out), C.byref(vel) if moving else None))
    d, at = dict(kind=kind), 0
    for name, w in fields:
        d[name] = out.v[at] if w == 1 else [out.v[at + i] for i in range(w)]
        at += w
    return (d, vel.tup()) if moving else d


def _contact_dict(c):
    return dict(a=c.a.tup(), b=c.b.tup(), n=c.n.tup(), t=c.t)


def contacts(ctx, a, vel_a, b, vel_b, cap=4):
    """Contacts::contacts (collision.rs:471-482) on the GPU for shape dicts a, b."""
    out = (Contact * cap)()
    n = C.c_int32()
    va = C.byref(_v3(vel_a)) if vel_a is not None else None
    vb = C.byref(_v3(vel_b)) if vel_b is not None else None
    _check(load_library().mgf_contacts(ctx._h, C.byref(_shape(a)), va, C.byref(_shape(b)), vb, out, cap, C.byref(n)))
    return [_contact_dict(out[i]) for i in range(n.value)]


def contacts_batch(ctx, problems):
    """problems: list of (a, vel_a, b, vel_b).  Returns a list of contact lists."""
    n = len(problems)
    A = (Shape * n)(*[_shape(p[0]) for p in problems])
    B = (Shape * n)(*[_shape(p[2]) for p in problems])
    va = np.zeros((n, 3), np.float32)
    vb = np.zeros((n, 3), np.float32)
    hv = np.zeros(n, np.uint8)
    for i, p in enumerate(problems):
        if p[1] is not None:
            va[i] = p[1]
            hv[i] |= 1
        if p[3] is not None:
            vb[i] = p[3]
            hv[i] |= 2
    out = (Contact * (2 * n))()
    counts = np.zeros(n, np.int32)
    _check(load_library().mgf_contacts_batch(ctx._h, n, A, va.ctypes.data, B, vb.ctypes.data, hv.ctypes.data, out,
                                             counts.ctypes.data))
    return [[_contact_dict(out[2 * i + k]) for k in range(counts[i])] for i in range(n)]


def tri_reject_batch(ctx, tag, p, d, r, delta, tris):
    """n (moving component, triangle) problems as arrays - tag (n,), p, d, delta (n, 3), r (n,), tris (n, 3, 3) - through the front end's cheap
    reject and through the body-triangle tests: returns (far (n,) uint8, counts (n,) int32)  (mgf_tri_reject_batch)."""
    n = len(tag)
    rec = np.zeros(n, dtype=np.dtype([("tag", np.int32), ("p", np.float32, 3), ("d", np.float32, 3), ("r", np.float32), ("delta", np.float32, 3)]))
    rec["tag"], rec["p"], rec["d"], rec["r"], rec["delta"] = tag, p, d, r, delta
    assert rec.dtype.itemsize == C.sizeof(MovingComponent)
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(n, 9)
    far = np.zeros(n, np.uint8)
    counts = np.zeros(n, np.int32)
    _check(load_library().mgf_tri_reject_batch(ctx._h, n, rec.ctypes.data, t.ctypes.data, far.ctypes.data, counts.ctypes.data))
    return far, counts


def _moving(tag, p, d, r, delta):
    return MovingComponent(Component(int(tag), _v3(p), _v3(d), float(r)), _v3(delta))


def _local_dict(lc):
    return dict(local_a=lc.local_a.tup(), local_b=lc.local_b.tup(), a=lc.glob.a.tup(), b=lc.glob.b.tup(),
                n=lc.glob.n.tup(), t=lc.glob.t)


def local_contacts_pair(ctx, a, b, cap=4):
    """LocalContacts for two Moving<Component>s given as (tag, p, d, r, delta) tuples (compound.rs:192-207)."""
    out = (LocalContact * cap)()
    n = C.c_int32()
    _check(load_library().mgf_local_contacts_pair(ctx._h, C.byref(_moving(*a)), C.byref(_moving(*b)), out, cap, C.byref(n)))
    return [_local_dict(out[i]) for i in range(n.value)]


def local_contacts_mesh(ctx, body, mesh, cap=32):
    out = (LocalContact * cap)()
    n = C.c_int32()
    _check(load_library().mgf_local_contacts_mesh(ctx._h, C.byref(_moving(*body)), mesh._h, out, cap, C.byref(n)))
    return [_local_dict(out[i]) for i in range(n.value)]


PARTICLE_DTYPE = np.dtype([("p", "<f4", 3), ("d", "<f4", 3), ("dt", "<f4")])
INTERSECTION_DTYPE = np.dtype([("p", "<f4", 3), ("t", "<f4")])


def particles(rays=(), segments=()):
    """Particles (geom.rs:802-855) from rays [(p, d)] and segments [(a, b)]: a Segment is p = a, d = b - a, DT = 1."""
    out = np.zeros(len(rays) + len(segments), PARTICLE_DTYPE)
    for i, (p, d) in enumerate(rays):
        out[i] = (p, d, np.inf)
    for i, (a, b) in enumerate(segments):
        a32, b32 = np.asarray(a, np.float32), np.asarray(b, np.float32)
        out[len(rays) + i] = (a32, b32 - a32, 1.0)
    return out


def intersections(ctx, parts, shapes=None, boxes=None):
    """Intersects<Shape> (shape dicts) or Intersects<AABB> (rows c3 r3) for each particle -> [(point, t) or None]."""
    parts = np.ascontiguousarray(parts, PARTICLE_DTYPE)
    n = len(parts)
    out = np.zeros(max(n, 1), INTERSECTION_DTYPE)
    hit = np.zeros(max(n, 1), np.int32)
    sp = bp = None
    if shapes is not None:
        arr = (Shape * max(n, 1))(*[_shape(x) for x in shapes])
        sp = C.cast(arr, C.c_void_p)
    else:
        bx = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
        bp = bx.ctypes.data
    _check(load_library().mgf_intersections_batch(ctx._h, n, parts.ctypes.data, sp, bp, out.ctypes.data, hit.ctypes.data))
    return [(tuple(float(v) for v in out[i]["p"]), float(out[i]["t"])) if hit[i] else None for i in range(n)]


def ray_capsule(ctx, p, d, cap_a, cap_d, cap_r):
    """Intersects<Capsule> for Ray (collision.rs:275-359) -> (point, t) or None."""
    ip = Vec3()
    t = C.c_float()
    hit = C.c_int32()
    s = _shape(dict(kind="capsule", a=cap_a, d=cap_d, r=cap_r))
    _check(load_library().mgf_ray_capsule(ctx._h, C.byref(_v3(p)), C.byref(_v3(d)), C.byref(s), C.byref(ip), C.byref(t), C.byref(hit)))
    return (ip.tup(), t.value) if hit.value else None


LOCAL_CONTACT_DTYPE = np.dtype([("local_a", "<f4", 3), ("local_b", "<f4", 3), ("a", "<f4", 3), ("b", "<f4", 3), ("n", "<f4", 3), ("t", "<f4")])
MANIFOLD_CAP = 8
MANIFOLD_DTYPE = np.dtype([("time", "<f4"), ("normal", "<f4", 3), ("tangent", "<f4", (2, 3)), ("n_contacts", "<i4"),
                           ("local_a", "<f4", (MANIFOLD_CAP, 3)), ("local_b", "<f4", (MANIFOLD_CAP, 3))])


def manifolds_from_contacts(ctx, offsets, contacts):
    """ContactPruner::push for each group's LocalContacts in order, then Manifold::from(pruner) (manifold.rs:42-148)."""
    offsets = np.ascontiguousarray(offsets, np.uint64)
    contacts = np.ascontiguousarray(contacts, LOCAL_CONTACT_DTYPE)
    n = len(offsets) - 1
    out = np.zeros(max(n, 1), MANIFOLD_DTYPE)
    _check(load_library().mgf_manifolds_from_contacts(ctx._h, None, n, offsets.ctypes.data, contacts.ctypes.data, out.ctypes.data))
    return out[:n]


def _to_json(fn, handle):
    n = C.c_int64()
    st = fn(handle, None, 0, C.byref(n))
    if st not in (OK, ERR_CAPACITY):
        _check(st)
    buf = C.create_string_buffer(n.value + 1)
    _check(fn(handle, buf, n.value + 1, C.byref(n)))
    return buf.value.decode()


CONTACT_DTYPE = np.dtype([("a", "<f4", 3), ("b", "<f4", 3), ("n", "<f4", 3), ("t", "<f4")])


class Compound:
    """mgf::Compound (compound.rs:230-352): comps = COMPONENT_DTYPE array (tag, p, d, r)."""

    def __init__(self, ctx, comps):
        self._h = C.c_void_p()
        self._ctx = ctx
        comps = np.ascontiguousarray(comps, COMPONENT_DTYPE)
        _check(load_library().mgf_compound_new(ctx._h if ctx is not None else None, comps.ctypes.data, len(comps), C.byref(self._h)))
        if ctx is not None:
            ctx._adopt(self)

    def __del__(self):
        if getattr(self, "_h", None):
            load_library().mgf_compound_free(self._h)
            self._h = None

    def set_pose(self, disp, rot):
        """rot = (s, x, y, z), assumed normalised"""
        _check(load_library().mgf_compound_set_pose(self._h, _v3(disp), Quat(*[float(v) for v in rot])))

    def bounds(self):
        b = Aabb()
        _check(load_library().mgf_compound_bounds(self._h, C.byref(b)))
        return b.c.tup(), b.r.tup()

    def contacts_many(self, moving):
        """moving = MOVING_DTYPE array of swept spheres / capsules -> (offsets, CONTACT_DTYPE array)"""
        moving = np.ascontiguousarray(moving, MOVING_DTYPE)
        n = len(moving)
        off = np.zeros(n + 1, np.uint64)
        total = C.c_int64()
        cap = max(4 * n, 16)
        while True:
            out = np.zeros(cap, CONTACT_DTYPE)
            st = load_library().mgf_compound_contacts_many(self._h, moving.ctypes.data, n, off.ctypes.data, out.ctypes.data, cap, C.byref(total))
            if st == ERR_CAPACITY and total.value > cap:
                cap = total.value
                continue
            _check(st)
            break
        return off.astype(np.int64), out[:total.value]

    def intersections(self, parts):
        parts = np.ascontiguousarray(parts, PARTICLE_DTYPE)
        n = len(parts)
        out = np.zeros(max(n, 1), INTERSECTION_DTYPE)
        hit = np.zeros(max(n, 1), np.int32)
        _check(load_library().mgf_compound_intersections(self._h, parts.ctypes.data, n, out.ctypes.data, hit.ctypes.data))
        return [(tuple(float(v) for v in out[i]["p"]), float(out[i]["t"])) if hit[i] else None for i in range(n)]


class Mesh:
    """mgf::Mesh (mesh.rs:32-73)."""

    def __init__(self, ctx):
        """ctx=None builds a host-only mesh (no device queries)."""
        self._ctx = ctx
        self._h = C.c_void_p()
        _check(load_library().mgf_mesh_new(ctx._h if ctx is not None else None, C.byref(self._h)))
        if ctx is not None:
            ctx._adopt(self)

    def __del__(self):
        if getattr(self, "_h", None):
            load_library().mgf_mesh_free(self._h)
            self._h = None

    def to_json(self):
        """serde_json shape of mgf::Mesh (mesh.rs:31-37)"""
        return _to_json(load_library().mgf_mesh_to_json, self._h)

    @classmethod
    def from_json(cls, ctx, text):
        self = cls.__new__(cls)
        self._ctx = ctx
        self._h = C.c_void_p()
        raw = text.encode()
        _check(load_library().mgf_mesh_from_json(ctx._h if ctx is not None else None, raw, len(raw), C.byref(self._h)))
        if ctx is not None:
            ctx._adopt(self)
        return self

    def push_vert(self, p):
        i = C.c_uint64()
        _check(load_library().mgf_mesh_push_vert(self._h, _v3(p), C.byref(i)))
        return i.value

    def push_face(self, a, b, c):
        i = C.c_uint64()
        _check(load_library().mgf_mesh_push_face(self._h, a, b, c, C.byref(i)))
        return i.value

    def set_pos(self, p):
        _check(load_library().mgf_mesh_set_pos(self._h, _v3(p)))

    def build(self, verts, faces):
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        faces = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
        _check(load_library().mgf_mesh_build(self._h, verts.ctypes.data, len(verts), faces.ctypes.data, len(faces)))

    def bvh_dump(self):
        view = load_library().mgf_mesh_bvh_view(self._h)
        return _bvh_dump(view)


def _bvh_dump(handle):
    L = load_library()
    n = L.mgf_bvh_dump(handle, None, None, 0)
    nodes = np.zeros((max(n, 1), 6), np.int64)
    boxes = np.zeros((max(n, 1), 6), np.float32)
    L.mgf_bvh_dump(handle, nodes.ctypes.data, boxes.ctypes.data, n)
    return nodes[:n], boxes[:n]


class Bvh:
    """mgf::BVH<AABB, usize> (bvh.rs:30-310)."""

    def __init__(self, ctx, capacity=None):
        self._ctx = ctx
        self._h = C.c_void_p()
        h = ctx._h if ctx is not None else None  # ctx=None: host-only tree (no device queries)
        if capacity is None:
            _check(load_library().mgf_bvh_new(h, C.byref(self._h)))
        else:
            _check(load_library().mgf_bvh_with_capacity(h, capacity, C.byref(self._h)))
        if ctx is not None:
            ctx._adopt(self)

    def __del__(self):
        if getattr(self, "_h", None):
            load_library().mgf_bvh_free(self._h)
            self._h = None

    def to_json(self):
        """serde_json shape of BVH<AABB, usize> (bvh.rs:29-47 over pool.rs:25-41)"""
        return _to_json(load_library().mgf_bvh_to_json, self._h)

    @classmethod
    def from_json(cls, ctx, text):
        self = cls.__new__(cls)
        self._ctx = ctx
        self._h = C.c_void_p()
        raw = text.encode()
        _check(load_library().mgf_bvh_from_json(ctx._h if ctx is not None else None, raw, len(raw), C.byref(self._h)))
        if ctx is not None:
            ctx._adopt(self)
        return self

    def empty(self):
        return bool(load_library().mgf_bvh_empty(self._h))

    def clear(self):
        _check(load_library().mgf_bvh_clear(self._h))

    def insert(self, c, r, val):
        i = C.c_uint64()
        _check(load_library().mgf_bvh_insert(self._h, C.byref(Aabb(_v3(c), _v3(r))), val, C.byref(i)))
        return i.value

    def remove(self, node):
        _check(load_library().mgf_bvh_remove(self._h, node))

    def root(self):
        i = C.c_uint64()
        _check(load_library().mgf_bvh_root(self._h, C.byref(i)))
        return i.value

    def get_leaf(self, node):
        v = C.c_uint64()
        _check(load_library().mgf_bvh_get_leaf(self._h, node, C.byref(v)))
        return v.value

    def bounds(self, node):
        a = Aabb()
        _check(load_library().mgf_bvh_bounds(self._h, node, C.byref(a)))
        return a.c.tup(), a.r.tup()

    def query(self, c, r):
        hits = []
        cb = HIT_FN(lambda pv, _u: hits.append(pv[0]))
        _check(load_library().mgf_bvh_query(self._h, C.byref(Aabb(_v3(c), _v3(r))), cb, None))
        return hits

    def query_many(self, boxes):
        boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
        n = len(boxes)
        off = np.zeros(n + 1, np.uint64)
        total = C.c_int64()
        cap = 1 << 16
        while True:
            vals = np.zeros(cap, np.uint64)
            st = load_library().mgf_bvh_query_many(self._h, boxes.ctypes.data, n, off.ctypes.data, vals.ctypes.data, cap, C.byref(total))
            if st == ERR_CAPACITY and total.value > cap:
                cap = total.value
                continue
            _check(st)
            break
        return off.astype(np.int64), vals[:total.value].astype(np.int64)

    def raytrace(self, p, d, dt=float("inf")):
        """BVH::raytrace (bvh.rs:345-369) for one particle through the callback form: [(value, point, t)] in the
        reference's visiting order."""
        part = np.zeros(1, PARTICLE_DTYPE)
        part["p"], part["d"], part["dt"] = p, d, dt
        hits = []

        def on_hit(pv, pi, _u):
            rec = np.ctypeslib.as_array(C.cast(pi, C.POINTER(C.c_float)), (4,))
            hits.append((int(pv[0]), (float(rec[0]), float(rec[1]), float(rec[2])), float(rec[3])))
        cb = RAY_FN(on_hit)
        _check(load_library().mgf_bvh_raytrace(self._h, part.ctypes.data, cb, None))
        return hits

    def raytrace_many(self, parts):
        """BVH::raytrace for each particle: (offsets, values, intersections with the leaf bounds)."""
        parts = np.ascontiguousarray(parts, PARTICLE_DTYPE)
        n = len(parts)
        off = np.zeros(n + 1, np.uint64)
        total = C.c_int64()
        cap = 1 << 16
        while True:
            vals = np.zeros(cap, np.uint64)
            inter = np.zeros(cap, INTERSECTION_DTYPE)
            st = load_library().mgf_bvh_raytrace_many(self._h, parts.ctypes.data, n, off.ctypes.data, vals.ctypes.data, inter.ctypes.data, cap,
                                                      C.byref(total))
            if st == ERR_CAPACITY and total.value > cap:
                cap = total.value
                continue
            _check(st)
            break
        return off.astype(np.int64), vals[:total.value].astype(np.int64), inter[:total.value]

    def dump(self):
        return _bvh_dump(self._h)


class Solver:
    """Solver<ContactConstraint> (solver.rs:53-79): an insertion-ordered constraint list that is solved on a World's
    RigidBodyVec; the constraints keep their accumulated impulses between solve calls."""

    def __init__(self):
        self._h = C.c_void_p()
        _check(load_library().mgf_solver_new(C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            load_library().mgf_solver_free(self._h)
            self._h = None

    def add_constraint(self, row):
        row = np.ascontiguousarray(row, CONSTRAINT_DTYPE).reshape(1)
        _check(load_library().mgf_solver_add_constraint(self._h, row.ctypes.data))

    def add_constraints(self, rows):
        rows = np.ascontiguousarray(rows, CONSTRAINT_DTYPE)
        _check(load_library().mgf_solver_add_constraints(self._h, rows.ctypes.data, len(rows)))

    def __len__(self):
        return load_library().mgf_solver_len(self._h)

    def clear(self):
        _check(load_library().mgf_solver_clear(self._h))

    def constraints(self):
        n = len(self)
        out = np.zeros(max(n, 1), CONSTRAINT_DTYPE)
        _check(load_library().mgf_solver_read_constraints(self._h, out.ctypes.data, len(out), None))
        return out[:n]

    def solve(self, world, iters):
        _check(load_library().mgf_solver_solve(self._h, world._h, int(iters), C.byref(world.stats)))
        return world.stats


# ---- marshalling shared by the queries of World and WorldBatch ------------------------------------------------------------------
def _per_query(v, n, optional=False, dtype=np.int32):
    """a value per query (world, ignore): a scalar or one row for all, or n rows; optional: None stays None (no ignore list)"""
    return None if optional and v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype), (n,)))


def _ptr(a):
    return None if a is None else a.ctypes.data


def _dev_arg(a, dtype, cols, n, name):
    """the address of a device-pointer call's argument: None, a raw integer address (taken as it is: the library checks that it is
    device memory and large enough), or a torch tensor - float32 / int32 as the call needs, contiguous, on a GPU, n rows of `cols`"""
    if a is None:
        return None
    if isinstance(a, (int, np.integer)):
        return int(a)
    if not hasattr(a, "data_ptr"):
        raise ValueError(f"{name}: a torch tensor on the GPU or an integer address, not {type(a).__name__}")
    if str(a.dtype) != "torch." + dtype:
        raise ValueError(f"{name}: dtype must be {dtype}, not {a.dtype}")
    if not a.is_contiguous():
        raise ValueError(f"{name}: the tensor is not contiguous")
    if a.numel() != n * cols or (a.dim() > 0 and a.shape[0] != n):
        raise ValueError(f"{name}: {tuple(a.shape)} is not {n} rows of {cols}")
    if a.device.type != "cuda":
        raise ValueError(f"{name}: the tensor is on {a.device}, not on the GPU")
    return int(a.data_ptr())


def _rig_rows(dtype, **fields):
    """a rig of `dtype` from its fields - arrays, or scalars / single rows for all: as many records as the longest argument has, none
    where an argument is empty; a field that is not given stays zero; ValueError where an argument is neither one nor n"""
    cols = {k: int(np.prod(dtype[k].shape, dtype=np.int64)) for k in fields}
    vals = {k: np.asarray(v, dtype[k].base) for k, v in fields.items()}
    n = 0 if min(v.size for v in vals.values()) == 0 else max(v.size // cols[k] for k, v in vals.items())
    rig = np.zeros(n, dtype)
    for k, v in vals.items():
        rig[k] = np.broadcast_to(v.reshape((-1,) + dtype[k].shape), (n,) + dtype[k].shape)
    return rig


def hinge_angles(readings):
    """(theta, rate) of hinge readings - a HINGE_READING_DTYPE or HINGE_TRACE_FULL_DTYPE array of any shape, as WorldBatch.read_hinges
    and hinge_trace return them: theta = arctan2(sn, c) in float64, radians in (-pi, pi]; rate in rad/s, float64"""
    r = np.asarray(readings)
    return np.arctan2(r["sn"].astype(np.float64), r["c"].astype(np.float64)), r["rate"].astype(np.float64)


def hinge_frames(a, b, anchor_world, axis_world):
    """pa, pb, ax, ua, bx, ub of hinges placed in the present pose: zero gap, parallel axes, theta = 0.  a: the state rows of every
    hinge's `body` - a mapping with "x" [n, 3] and "q" [n, 4] (scalar first), and "delta" where x + delta is the pose, as state()
    returns them; b: the same of `other`, or None where every far end is the world (a row of b whose q is all zero is the world too).
    anchor_world [n, 3] and axis_world [n, 3] (any length but zero) in the world's frame.  Works in float64 and rounds once.  Returns
    a dict of float32 [n, 3] arrays, ready for WorldBatch.set_hinges(**frames)."""
    d = np.float64

    def pose(s):
        x = np.asarray(s["x"], np.float32).reshape(-1, 3)
        names = (s.dtype.names or ()) if isinstance(s, np.ndarray) else s
        if "delta" in names:
            x = x + np.asarray(s["delta"], np.float32).reshape(-1, 3)      # (the state's own f32 sum, as gather_state returns it)
        return x.astype(d), np.asarray(s["q"], d).reshape(-1, 4)

    def local(x, q, p, point):
        world = ~np.any(q != 0, axis=1)
        s, v = q[:, 0:1], -q[:, 1:4]
        r = p - x if point else p
        out = np.cross(v, np.cross(v, r) + r * s) * 2.0 + r
        return np.where(world[:, None], p, out)
    anchor = np.asarray(anchor_world, d).reshape(-1, 3)
    axis = np.asarray(axis_world, d).reshape(-1, 3)
    axis = axis / np.linalg.norm(axis, axis=1, keepdims=True)
    least = np.eye(3)[np.argmin(np.abs(axis), axis=1)]                      # the coordinate axis the hinge axis leans on least
    ref = np.cross(axis, least)
    ref = ref / np.linalg.norm(ref, axis=1, keepdims=True)
    xa, qa = pose(a)
    n = len(xa)
    anchor, axis, ref = (np.broadcast_to(t, (n, 3)) for t in (anchor, axis, ref))
    xb, qb = pose(b) if b is not None else (np.zeros((n, 3)), np.zeros((n, 4)))
    out = {"pa": local(xa, qa, anchor, True), "ax": local(xa, qa, axis, False), "ua": local(xa, qa, ref, False),
           "pb": local(xb, qb, anchor, True), "bx": local(xb, qb, axis, False), "ub": local(xb, qb, ref, False)}
    return {k: v.astype(np.float32) for k, v in out.items()}


def slider_frames(a, b, anchor_world, axis_world):
    """pa, pb, ax, ua, bx, ub of sliders placed in the present pose: zero gap, aligned frames, travel d = 0.  The arguments are
    hinge_frames': a and b the state rows of every slider's `body` and `other` (b None, or a row whose q is all zero: the world),
    anchor_world [n, 3] and axis_world [n, 3] - the slide axis, any length but zero - in the world's frame.  Works in float64 and
    rounds once.  Returns a dict of float32 [n, 3] arrays, ready for WorldBatch.set_sliders(**frames)."""
    return hinge_frames(a, b, anchor_world, axis_world)


def _record_k(out, k):
    """the k of records of 1 + k words: out.shape[1] - 1 of a tensor, or as given with a raw address"""
    if k is None:
        if not hasattr(out, "data_ptr") or out.dim() != 2 or out.shape[1] < 1:
            raise ValueError("out: a tensor of n rows of 1 + k, or k given with a raw address")
        k = int(out.shape[1]) - 1
    return int(k)


def _particle_rows(p, d, dt):
    """mgf_particle rows (p.xyz, d.xyz, dt) from rows of p; d and dt are rows, or one for all"""
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    parts = np.empty((len(p), 7), np.float32)
    parts[:, 0:3] = p
    parts[:, 3:6] = np.broadcast_to(np.asarray(d, np.float32), p.shape)
    parts[:, 6] = np.broadcast_to(np.asarray(dt, np.float32), (len(p),))
    return parts


def _cast_rows(comps, delta):
    """MOVING_DTYPE rows from COMPONENT_DTYPE rows swept by delta (rows, or one vector for all), or from a MOVING_DTYPE array as it is"""
    comps = np.asarray(comps)
    if comps.dtype == MOVING_DTYPE:
        if delta is not None:
            raise ValueError("a MOVING_DTYPE array carries its own delta")
        return np.ascontiguousarray(comps.reshape(-1))
    comps = np.asarray(comps, COMPONENT_DTYPE).reshape(-1)
    casts = np.zeros(len(comps), MOVING_DTYPE)
    for k in ("tag", "p", "d", "r"):
        casts[k] = comps[k]
    casts["delta"] = np.broadcast_to(np.asarray(0.0 if delta is None else delta, np.float32), (len(comps), 3))
    return casts


def _boxes_from_corners(lo, hi):
    """mgf_aabb rows c = (hi + lo) / 2, r = (hi - lo) / 2 in f32"""
    lo = np.asarray(lo, np.float32).reshape(-1, 3)
    hi = np.asarray(hi, np.float32).reshape(-1, 3)
    boxes = np.empty((len(lo), 6), np.float32)
    boxes[:, 0:3] = (hi + lo) / np.float32(2)
    boxes[:, 3:6] = (hi - lo) / np.float32(2)
    return boxes


def _overlap_lists(call, n, cap):
    """(offsets[n + 1], bodies) of call(off, vals, cap, total) - an overlap entry point with everything but its output bound; cap None
    sizes the output from a first call's count"""
    off = np.zeros(n + 1, np.uint64)
    total = C.c_int64()
    if cap is None:
        st = call(off.ctypes.data, None, 0, C.byref(total))
        if st not in (0, ERR_CAPACITY):
            _check(st)
        cap = total.value
    vals = np.zeros(max(int(cap), 1), np.uint32)
    _check(call(off.ctypes.data, vals.ctypes.data, int(cap), C.byref(total)))
    return off.astype(np.int64), vals[:total.value].copy()


class World:
    """RigidBodyVec + Solver + terrain + broadphase resident on one GPU; `step` is
    mgf_demo/world.rs::World::step."""

    def __init__(self, ctx, params=None):
        self._ctx = ctx
        self._h = C.c_void_p()
        self.stats = StepStats()
        p = C.byref(params) if params is not None else None
        _check(load_library().mgf_world_new(ctx._h, p, C.byref(self._h)))
        ctx._adopt(self)

    def __del__(self):
        if getattr(self, "_h", None):
            load_library().mgf_world_free(self._h)
            self._h = None

    @classmethod
    def from_scene(cls, ctx, scene, params=None):
        w = cls(ctx, params)
        t = scene["terrain"]
        if t is not None:
            m = Mesh(ctx)
            m.build(t["verts"], t["faces"])
            m.set_pos(t["pos"])
            w.set_terrain(m)
        if len(scene["comps"]):
            w.add_bodies(scene["comps"], scene["mass"], scene["restitution"], scene["friction"], scene["force"])
        cb = scene.get("compound")  # bodies of several components, appended after the ordinary ones
        if cb is not None:
            w.add_compound_bodies(cb["comps"], cb["comp_mass"], cb["offsets"], cb["restitution"], cb["friction"], cb["force"])
        if scene.get("v0") is not None:
            w.write_state(v=scene["v0"])
        return w

    def set_terrain(self, mesh):
        _check(load_library().mgf_world_set_terrain(self._h, mesh._h if mesh is not None else None))

    def add_obstacle(self, compound):
        """A static Compound as an obstacle of the world beside the Mesh (mgf_world_add_obstacle; the compound is copied)."""
        _check(load_library().mgf_world_add_obstacle(self._h, compound._h))

    def add_bodies(self, comps, mass, restitution, friction, world_force):
        comps = np.ascontiguousarray(comps, dtype=COMPONENT_DTYPE)
        n = len(comps)
        mass = np.ascontiguousarray(np.broadcast_to(np.asarray(mass, np.float32), (n,)))
        rest = np.ascontiguousarray(np.broadcast_to(np.asarray(restitution, np.float32), (n,)))
        fric = np.ascontiguousarray(np.broadcast_to(np.asarray(friction, np.float32), (n,)))
        force = np.ascontiguousarray(np.broadcast_to(np.asarray(world_force, np.float32), (n, 3)))
        first = C.c_uint64()
        _check(load_library().mgf_world_add_bodies(self._h, comps.ctypes.data, n, mass.ctypes.data, rest.ctypes.data,
                                                   fric.ctypes.data, force.ctypes.data, C.byref(first)))
        return first.value

    def add_compound_bodies(self, comps, comp_mass, offsets, restitution, friction, world_force):
        """Bodies of several components (mgf_world_add_compound_bodies): body b = comps[offsets[b]:offsets[b + 1]]."""
        comps = np.ascontiguousarray(comps, dtype=COMPONENT_DTYPE)
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        cm = np.ascontiguousarray(np.broadcast_to(np.asarray(comp_mass, np.float32), (len(comps),)))
        rest = np.ascontiguousarray(np.broadcast_to(np.asarray(restitution, np.float32), (n,)))
        fric = np.ascontiguousarray(np.broadcast_to(np.asarray(friction, np.float32), (n,)))
        force = np.ascontiguousarray(np.broadcast_to(np.asarray(world_force, np.float32), (n, 3)))
        first = C.c_uint64()
        _check(load_library().mgf_world_add_compound_bodies(self._h, comps.ctypes.data, cm.ctypes.data, offsets.ctypes.data, n,
                                                            rest.ctypes.data, fric.ctypes.data, force.ctypes.data, C.byref(first)))
        return first.value

    def __len__(self):
        return load_library().mgf_world_len(self._h)

    def step(self, dt, iters):
        _check(load_library().mgf_world_step(self._h, float(dt), int(iters), C.byref(self.stats)))
        return self.stats

    def step_many(self, dt, iters, n):
        """n ticks in one call; returns the per-tick statistics (a ctypes array of StepStats)."""
        arr = (StepStats * int(n))()
        _check(load_library().mgf_world_step_many(self._h, float(dt), int(iters), int(n), arr))
        if n:
            self.stats = arr[int(n) - 1]
        return arr

    def build_constraints(self, dt):
        _check(load_library().mgf_world_build_constraints(self._h, float(dt), C.byref(self.stats)))
        return self.stats

    def solve(self, iters):
        _check(load_library().mgf_world_solve(self._h, int(iters), C.byref(self.stats)))
        return self.stats

    def complete_motion(self):
        _check(load_library().mgf_world_complete_motion(self._h))

    def integrate(self, dt):
        _check(load_library().mgf_world_integrate(self._h, float(dt)))

    def get(self, index=None, static=None):
        """ConstrainedSet::get: index for Dynamic(i), static=(center, friction) for Static."""
        ref = BodyRef(0, index, Vec3(), 0.0) if static is None else BodyRef(1, 0, _v3(static[0]), float(static[1]))
        vel, info = Velocity(), RigidBodyInfo()
        _check(load_library().mgf_world_get(self._h, C.byref(ref), C.byref(vel), C.byref(info)))
        return vel, info

    def set(self, index, linear, angular):
        ref = BodyRef(0, index, Vec3(), 0.0)
        vel = Velocity(_v3(linear), _v3(angular))
        _check(load_library().mgf_world_set(self._h, C.byref(ref), C.byref(vel)))

    def state(self):
        n = len(self)
        x = np.empty((n, 3), np.float32)  # (every element is written: mgf_world_read_state fills n bodies)
        q = np.empty((n, 4), np.float32)
        v = np.empty((n, 3), np.float32)
        w = np.empty((n, 3), np.float32)
        d = np.empty((n, 3), np.float32)
        _check(load_library().mgf_world_read_state(self._h, x.ctypes.data, q.ctypes.data, v.ctypes.data, w.ctypes.data,
                                                   d.ctypes.data, n))
        return dict(x=x, q=q, v=v, omega=w, delta=d)

    def write_state(self, x=None, q=None, v=None, omega=None, delta=None):
        keep = []

        def p(a, k):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float32).reshape(-1, k)
            assert len(a) == len(self)
            keep.append(a)
            return a.ctypes.data
        _check(load_library().mgf_world_write_state(self._h, p(x, 3), p(q, 4), p(v, 3), p(omega, 3), p(delta, 3), len(self)))

    def colliders(self):
        out = np.zeros(len(self), MOVING_DTYPE)
        _check(load_library().mgf_world_read_colliders(self._h, out.ctypes.data, len(out)))
        return out

    def raycast(self, p, d, dt=float("inf"), ignore=None, kinds=QUERY_ALL):
        """Closest hit of each particle (rows of p, d; dt = inf: a Ray, 1: a Segment from p to p + d) against the bodies, the terrain
        and the obstacles (mgf_world_raycast_many): a RAY_HIT_DTYPE array, kind HIT_NONE where nothing is hit.  ignore: None or a
        caller body index per particle (-1: none); kinds: QUERY_* bits."""
        parts = _particle_rows(p, d, dt)
        ign = _per_query(ignore, len(parts), optional=True)
        out = np.zeros(len(parts), RAY_HIT_DTYPE)
        _check(load_library().mgf_world_raycast_many(self._h, parts.ctypes.data, len(parts), _ptr(ign), int(kinds), out.ctypes.data))
        return out

    def sweep(self, comps, delta=None, ignore=None, kinds=QUERY_ALL):
        """Earliest contact of each swept sphere or capsule against the bodies, the terrain and the obstacles (mgf_world_sweep_many): a
        SWEEP_HIT_DTYPE array, kind HIT_NONE where nothing is met.  comps: COMPONENT_DTYPE rows swept by delta (rows, or one vector for
        all), or a MOVING_DTYPE array that carries its own delta (then delta is None); ignore: None or a caller body index per cast
        (-1: none); kinds: QUERY_* bits."""
        casts = _cast_rows(comps, delta)
        ign = _per_query(ignore, len(casts), optional=True)
        out = np.zeros(len(casts), SWEEP_HIT_DTYPE)
        _check(load_library().mgf_world_sweep_many(self._h, casts.ctypes.data, len(casts), _ptr(ign), int(kinds), out.ctypes.data))
        return out

    def overlap_aabb(self, lo, hi):
        """The bodies whose tight box overlaps each box [lo, hi] (rows; mgf_world_overlap_aabb_many): (offsets[n + 1], bodies) in CSR
        form, each list in ascending caller index.  The box handed over is the mgf_aabb c = (hi + lo) / 2, r = (hi - lo) / 2 in f32."""
        return self.overlap_boxes(_boxes_from_corners(lo, hi))

    def overlap_boxes(self, boxes, cap=None):
        """overlap_aabb for mgf_aabb rows (c.xyz, r.xyz) as given; cap None sizes the output from a first call's count."""
        boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
        fn = load_library().mgf_world_overlap_aabb_many
        return _overlap_lists(lambda *o: fn(self._h, boxes.ctypes.data, len(boxes), *o), len(boxes), cap)

    def constraints(self):
        n = C.c_int64()
        _check(load_library().mgf_world_read_constraints(self._h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), CONSTRAINT_DTYPE)
        _check(load_library().mgf_world_read_constraints(self._h, out.ctypes.data, len(out), C.byref(n)))
        return out[:n.value]

    def set_constraints(self, cons):
        cons = np.ascontiguousarray(cons, CONSTRAINT_DTYPE)
        _check(load_library().mgf_world_set_constraints(self._h, cons.ctypes.data, len(cons)))

    def clone(self):
        """RigidBodyVec: Clone (physics.rs:140) with the world around it: an independent world that steps identically."""
        w = World.__new__(World)
        w._ctx, w._h, w.stats = self._ctx, C.c_void_p(), StepStats()
        _check(load_library().mgf_world_clone(self._h, C.byref(w._h)))
        self._ctx._adopt(w)
        return w

    def constraints_new(self, refs_a, refs_b, manifolds, dt):
        """ContactConstraint::new (solver.rs:101-191) for caller-built manifolds: refs are body indices (obj_b: an index, or
        (center, friction) for RigidBodyRef::Static); manifolds a MANIFOLD_DTYPE array.  -> flattened CONSTRAINT_DTYPE rows."""
        manifolds = np.ascontiguousarray(manifolds, MANIFOLD_DTYPE)
        n = len(manifolds)
        ra = (BodyRef * max(n, 1))()
        rb = (BodyRef * max(n, 1))()
        for i in range(n):
            a, b = refs_a[i], refs_b[i]
            ra[i] = BodyRef(0, int(a), Vec3(), 0.0) if not isinstance(a, tuple) else BodyRef(1, 0, _v3(a[0]), float(a[1]))
            rb[i] = BodyRef(0, int(b), Vec3(), 0.0) if not isinstance(b, tuple) else BodyRef(1, 0, _v3(b[0]), float(b[1]))
        cap = int(manifolds["n_contacts"].sum()) if n else 0
        out = np.zeros(max(cap, 1), CONSTRAINT_DTYPE)
        cnt = C.c_int64()
        _check(load_library().mgf_constraints_new(self._h, ra, rb, manifolds.ctypes.data, n, float(dt), out.ctypes.data, cap, C.byref(cnt)))
        return out[:cnt.value]

    # ---- tiling (device pointers of the caller) ----
    def begin_tick(self, dt):
        _check(load_library().mgf_world_begin_tick(self._h, float(dt)))

    def collide(self, dt):
        _check(load_library().mgf_world_collide(self._h, float(dt), C.byref(self.stats)))
        return self.stats

    def select_boundary(self, x_left, x_right, ids_left_ptr, ids_right_ptr, cap):
        nl, nr = C.c_int64(), C.c_int64()
        _check(load_library().mgf_world_select_boundary(self._h, float(x_left), float(x_right), ids_left_ptr, ids_right_ptr,
                                                        int(cap), C.byref(nl), C.byref(nr)))
        return nl.value, nr.value

    def export_bodies(self, ids_ptr, n, dst_ptr):
        _check(load_library().mgf_world_export_bodies(self._h, ids_ptr, int(n), dst_ptr))

    def import_ghosts(self, src_ptr, n):
        _check(load_library().mgf_world_import_ghosts(self._h, src_ptr, int(n)))

    def export_velocities(self, ids_ptr, n, dst_ptr):
        _check(load_library().mgf_world_export_velocities(self._h, ids_ptr, int(n), dst_ptr))

    def import_ghost_velocities(self, src_ptr, n):
        _check(load_library().mgf_world_import_ghost_velocities(self._h, src_ptr, int(n)))

    def ghost_len(self):
        return load_library().mgf_world_ghost_len(self._h)

    # ---- migration between tiles (device pointers, like the ghost calls) ----
    def select_tile(self, x_left, x_right, x_lo, x_hi, ids_left_ptr, ids_right_ptr, ids_migrants_ptr, cap):
        """-> (n_boundary_left, n_boundary_right, n_migrants_left, n_migrants_right)"""
        counts = (C.c_int64 * 4)()
        _check(load_library().mgf_world_select_tile(self._h, float(x_left), float(x_right), float(x_lo), float(x_hi), ids_left_ptr,
                                                    ids_right_ptr, ids_migrants_ptr, int(cap), counts))
        return tuple(int(c) for c in counts)

    def export_migrants(self, ids_ptr, n, dst_ptr):
        _check(load_library().mgf_world_export_migrants(self._h, ids_ptr, int(n), dst_ptr))

    def remove_bodies(self, ids_ptr, n):
        _check(load_library().mgf_world_remove_bodies(self._h, ids_ptr, int(n)))

    def import_migrants(self, src_ptr, n):
        _check(load_library().mgf_world_import_migrants(self._h, src_ptr, int(n)))

    def set_tags(self, tags):
        tags = np.ascontiguousarray(tags, np.uint32)
        _check(load_library().mgf_world_set_tags(self._h, tags.ctypes.data, len(tags)))

    def tags(self):
        out = np.zeros(max(len(self), 1), np.uint32)
        _check(load_library().mgf_world_read_tags(self._h, out.ctypes.data, len(out)))
        return out[:len(self)].copy()

    def solve_enqueue(self, iters):
        _check(load_library().mgf_world_solve_enqueue(self._h, int(iters)))

    def finish(self):
        _check(load_library().mgf_world_finish(self._h, C.byref(self.stats)))
        return self.stats

    def counter(self, name):
        v = C.c_int64()
        _check(load_library().mgf_world_counter(self._h, name.encode(), C.byref(v)))
        return v.value

    def set_option(self, key, value):
        _check(load_library().mgf_world_set_option(self._h, key.encode(), int(value)))

    def device_ptr(self, name):
        p = C.c_void_p()
        nb = C.c_int64()
        _check(load_library().mgf_world_device_ptr(self._h, name.encode(), C.byref(p), C.byref(nb)))
        return p.value, nb.value

    def release_device_ptrs(self):
        _check(load_library().mgf_world_release_device_ptrs(self._h))


def terrain_table(terrains):
    """The terrain table of WorldBatch.from_scenes(own_terrain=True) for one scene terrain (dict of verts, faces, pos, or None) per
    world: (entries, assignment) - the distinct geometries in the order they first occur, each at its first position, and per world
    (entry id or -1, pos).  Terrains with the same vertices and faces, bit for bit, share an entry whatever their pos."""
    entries, ids, assign = [], {}, []
    for t in terrains:
        if t is None:
            assign.append((-1, (0.0, 0.0, 0.0)))
            continue
        v = np.ascontiguousarray(t["verts"], np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(t["faces"], np.uint32).reshape(-1, 3)
        key = (v.shape[0], f.shape[0], v.tobytes(), f.tobytes())
        if key not in ids:
            ids[key] = len(entries)
            entries.append(t)
        assign.append((ids[key], tuple(float(c) for c in t["pos"])))
    return entries, assign


class WorldBatch:
    """Many small independent worlds resident on one GPU, stepped together (mgf_batch_*): per world `step` is
    mgf_demo/world.rs::World::step, one workgroup a world.  At most BATCH_MAX_BODIES bodies of one to four components per world
    (add_compound_bodies; on a batch that holds a body of more than one component the calls that read the shapes of bodies - ray
    casts, sweeps, box overlaps, sensors, cameras, zones, feelers - raise ERR_INVALID: they do not see parts yet); a world's
    terrain is an entry of the batch's terrain table (shared by any number of worlds) at a position of its own, or none; its static
    Compound obstacles are a list of entries of the batch's obstacle table, each at a pose of the world's own."""

    def __init__(self, ctx, n_worlds, params=None):
        self._ctx = ctx
        self._h = C.c_void_p()
        self.n_worlds = int(n_worlds)
        p = C.byref(params) if params is not None else None
        _check(load_library().mgf_batch_new(ctx._h, p, self.n_worlds, C.byref(self._h)))
        ctx._adopt(self)

    def __del__(self):
        if getattr(self, "_h", None):
            load_library().mgf_batch_free(self._h)
            self._h = None

    @classmethod
    def from_scenes(cls, ctx, scenes, params=None, own_terrain=False):
        """scenes as mgf_amd.scenes makes them, one per world; the first scene's terrain serves all, or (own_terrain) every world gets
        its scene's: scenes whose terrains have the same vertices and faces share a table entry, each at its own `pos`.  A scene may
        carry "obstacles": a list of (comps, disp, rot) - static Compounds of COMPONENT_DTYPE rows at a pose (rot = (s, x, y, z)), in
        the order the tick meets them; compounds with the same components, bit for bit, share an entry of the obstacle table"""
        b = cls(ctx, len(scenes), params)
        if own_terrain:
            entry, pos = terrain_table([sc["terrain"] for sc in scenes])
            for t in entry:
                m = Mesh(ctx)
                m.build(t["verts"], t["faces"])
                m.set_pos(t["pos"])
                b.add_terrain(m)
            if len(scenes):
                b.set_world_terrain(np.arange(len(scenes)), [e for e, _ in pos], [p for _, p in pos])
        else:
            t = scenes[0]["terrain"] if len(scenes) else None
            if t is not None:
                m = Mesh(ctx)
                m.build(t["verts"], t["faces"])
                m.set_pos(t["pos"])
                b.set_terrain(m)
        ids, rec = {}, []
        for k, sc in enumerate(scenes):
            for comps, disp, rot in (sc.get("obstacles") or ()):
                comps = np.ascontiguousarray(comps, COMPONENT_DTYPE)
                key = (len(comps), comps.tobytes())
                if key not in ids:
                    ids[key] = b.add_obstacle(Compound(ctx, comps))
                rec.append((k, ids[key], tuple(float(c) for c in disp), tuple(float(c) for c in rot)))
        if rec:
            b.set_world_obstacles([r[0] for r in rec], [r[1] for r in rec], [r[2] for r in rec], [r[3] for r in rec])
        for k, sc in enumerate(scenes):
            if len(sc["comps"]):
                b.add_bodies(k, sc["comps"], sc["mass"], sc["restitution"], sc["friction"], sc["force"])
            cb = sc.get("compound")  # bodies of up to four components, behind the ordinary ones (World.from_scene)
            if cb is not None:
                b.add_compound_bodies(k, cb["comps"], cb["comp_mass"], cb["offsets"], cb["restitution"], cb["friction"], cb["force"])
            if sc.get("v0") is not None and b.world_len(k):
                b.write_state(k, v=sc["v0"])
        return b

    def set_terrain(self, mesh):
        """the table emptied, `mesh` its entry 0 and every world's terrain; None: no world has terrain"""
        _check(load_library().mgf_batch_set_terrain(self._h, mesh._h if mesh is not None else None))

    def add_terrain(self, mesh):
        """a copy of the mesh (at its current position) as a new entry of the terrain table; returns its id.  No world changes."""
        i = C.c_int32(-1)
        _check(load_library().mgf_batch_add_terrain(self._h, mesh._h if mesh is not None else None, C.byref(i)))
        return i.value

    def set_world_terrain(self, world, terrain, pos=None):
        """world[i] gets table entry terrain[i] (-1: none) at pos[i] (None: where the mesh was when it was added), from the next tick;
        scalars or arrays (a scalar terrain, one pos: for every world named)"""
        wd = np.ascontiguousarray(np.atleast_1d(world), np.int32)
        n = len(wd)
        tr = np.ascontiguousarray(np.broadcast_to(np.asarray(terrain, np.int32), (n,)))
        ps = None if pos is None else np.ascontiguousarray(np.broadcast_to(np.asarray(pos, np.float32), (n, 3)))
        _check(load_library().mgf_batch_set_world_terrain(self._h, wd.ctypes.data, tr.ctypes.data, _ptr(ps), n))

    def terrain_count(self):
        return load_library().mgf_batch_terrain_count(self._h)

    def add_obstacle(self, compound):
        """a copy of the Compound (components, tree and current pose) as a new entry of the obstacle table; returns its id.  No world
        changes."""
        i = C.c_int32(-1)
        _check(load_library().mgf_batch_add_obstacle(self._h, compound._h if compound is not None else None, C.byref(i)))
        return i.value

    def set_world_obstacles(self, world, obstacle, disp=None, rot=None):
        """every world some record names gets its list of obstacles replaced by its records, in array order, from the next tick:
        record i puts table entry obstacle[i] (-1: nothing - a world named only so ends with an empty list) at disp[i], rot[i] =
        (s, x, y, z) taken as normalised (None, each on its own: the pose the compound had when it was added) into world[i]'s list.
        Scalars or arrays (a scalar world or obstacle, one disp, one rot: for every record)"""
        n = max(np.size(world), np.size(obstacle))
        wd = np.ascontiguousarray(np.broadcast_to(np.asarray(world, np.int32), (n,)))
        ob = np.ascontiguousarray(np.broadcast_to(np.asarray(obstacle, np.int32), (n,)))
        dp = None if disp is None else np.ascontiguousarray(np.broadcast_to(np.asarray(disp, np.float32), (n, 3)))
        rt = None if rot is None else np.ascontiguousarray(np.broadcast_to(np.asarray(rot, np.float32), (n, 4)))
        _check(load_library().mgf_batch_set_world_obstacles(self._h, wd.ctypes.data, ob.ctypes.data, _ptr(dp), _ptr(rt), n))

    def obstacle_count(self):
        return load_library().mgf_batch_obstacle_count(self._h)

    def world_obstacle_count(self, world):
        return load_library().mgf_batch_world_obstacle_count(self._h, int(world))

    def add_bodies(self, world, comps, mass, restitution, friction, world_force):
        comps = np.ascontiguousarray(comps, dtype=COMPONENT_DTYPE)
        n = len(comps)
        mass = np.ascontiguousarray(np.broadcast_to(np.asarray(mass, np.float32), (n,)))
        rest = np.ascontiguousarray(np.broadcast_to(np.asarray(restitution, np.float32), (n,)))
        fric = np.ascontiguousarray(np.broadcast_to(np.asarray(friction, np.float32), (n,)))
        force = np.ascontiguousarray(np.broadcast_to(np.asarray(world_force, np.float32), (n, 3)))
        first = C.c_uint64()
        _check(load_library().mgf_batch_add_bodies(self._h, int(world), comps.ctypes.data, n, mass.ctypes.data, rest.ctypes.data,
                                                   fric.ctypes.data, force.ctypes.data, C.byref(first)))
        return first.value

    def add_compound_bodies(self, world, comps, comp_mass, offsets, restitution, friction, world_force):
        """Bodies of 1..4 components for one world (mgf_batch_add_compound_bodies): body r = comps[offsets[r]:offsets[r + 1]], as
        World.add_compound_bodies; a body of one component is the ordinary body.  Returns the first new body's index in the world."""
        comps = np.ascontiguousarray(comps, dtype=COMPONENT_DTYPE)
        offsets = np.ascontiguousarray(offsets, np.int64)
        n = len(offsets) - 1
        cm = np.ascontiguousarray(np.broadcast_to(np.asarray(comp_mass, np.float32), (len(comps),)))
        rest = np.ascontiguousarray(np.broadcast_to(np.asarray(restitution, np.float32), (n,)))
        fric = np.ascontiguousarray(np.broadcast_to(np.asarray(friction, np.float32), (n,)))
        force = np.ascontiguousarray(np.broadcast_to(np.asarray(world_force, np.float32), (n, 3)))
        first = C.c_uint64()
        _check(load_library().mgf_batch_add_compound_bodies(self._h, int(world), comps.ctypes.data, cm.ctypes.data, offsets.ctypes.data, n,
                                                            rest.ctypes.data, fric.ctypes.data, force.ctypes.data, C.byref(first)))
        return first.value

    def __len__(self):
        return load_library().mgf_batch_len(self._h, -1)

    def world_len(self, world):
        return load_library().mgf_batch_len(self._h, int(world))

    def step(self, dt, iters, n=1):
        """n ticks of every world in one call; returns the statistics, arr[t * n_worlds + k] = world k's tick t"""
        arr = (StepStats * (int(n) * self.n_worlds))()
        _check(load_library().mgf_batch_step(self._h, float(dt), int(iters), int(n), arr))
        return arr

    def state(self, world=None):
        """x, q, v, omega, delta of one world, or (world=None) of the whole batch, worlds concatenated in order"""
        w = -1 if world is None else int(world)
        n = max(load_library().mgf_batch_len(self._h, w), 0)
        a = {k: np.empty((n, 4 if k == "q" else 3), np.float32) for k in ("x", "q", "v", "omega", "delta")}
        _check(load_library().mgf_batch_read_state(self._h, w, a["x"].ctypes.data, a["q"].ctypes.data, a["v"].ctypes.data,
                                                   a["omega"].ctypes.data, a["delta"].ctypes.data, n))
        return a

    def write_state(self, world, x=None, q=None, v=None, omega=None, delta=None):
        """the given arrays of one world (None: of the whole batch); no other world is touched"""
        w = -1 if world is None else int(world)
        n = max(load_library().mgf_batch_len(self._h, w), 0)
        keep = []

        def p(a, k):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float32).reshape(-1, k)
            assert len(a) == n
            keep.append(a)
            return a.ctypes.data
        _check(load_library().mgf_batch_write_state(self._h, w, p(x, 3), p(q, 4), p(v, 3), p(omega, 3), p(delta, 3), n))

    def constraints(self, world):
        cnt = C.c_int64()
        _check(load_library().mgf_batch_read_constraints(self._h, int(world), None, 0, C.byref(cnt)))
        out = np.zeros(cnt.value, CONSTRAINT_DTYPE)
        _check(load_library().mgf_batch_read_constraints(self._h, int(world), out.ctypes.data, len(out), C.byref(cnt)))
        return out

    def colliders(self, world=None):
        """the collider a query sees and the body's delta (MOVING_DTYPE) of one world, or (world=None) of the whole batch"""
        w = -1 if world is None else int(world)
        out = np.zeros(max(load_library().mgf_batch_len(self._h, w), 0), MOVING_DTYPE)
        _check(load_library().mgf_batch_read_colliders(self._h, w, out.ctypes.data, len(out)))
        return out

    def raycast(self, world, p, d, dt=float("inf"), ignore=None, kinds=QUERY_ALL):
        """As World.raycast, particle i against world[i] (a scalar: all against that world) of the batch (mgf_batch_raycast_many): a
        RAY_HIT_DTYPE array; index and ignore are body indices within the particle's world."""
        parts = _particle_rows(p, d, dt)
        wd, ign = _per_query(world, len(parts)), _per_query(ignore, len(parts), optional=True)
        out = np.zeros(len(parts), RAY_HIT_DTYPE)
        _check(load_library().mgf_batch_raycast_many(self._h, wd.ctypes.data, parts.ctypes.data, len(parts), _ptr(ign), int(kinds), out.ctypes.data))
        return out

    def sweep(self, world, comps, delta=None, ignore=None, kinds=QUERY_ALL):
        """As World.sweep, cast i against world[i] (a scalar: all against that world) of the batch (mgf_batch_sweep_many): a
        SWEEP_HIT_DTYPE array; index and ignore are body indices within the cast's world."""
        casts = _cast_rows(comps, delta)
        wd, ign = _per_query(world, len(casts)), _per_query(ignore, len(casts), optional=True)
        out = np.zeros(len(casts), SWEEP_HIT_DTYPE)
        _check(load_library().mgf_batch_sweep_many(self._h, wd.ctypes.data, casts.ctypes.data, len(casts), _ptr(ign), int(kinds), out.ctypes.data))
        return out

    def body_contacts(self, world=None):
        """the last tick's constraint list folded per body (mgf_batch_read_body_contacts): a BODY_CONTACTS_DTYPE array for one world, or
        (world=None) for the whole batch, worlds concatenated in order"""
        w = -1 if world is None else int(world)
        out = np.zeros(max(load_library().mgf_batch_len(self._h, w), 0), BODY_CONTACTS_DTYPE)
        _check(load_library().mgf_batch_read_body_contacts(self._h, w, out.ctypes.data, len(out)))
        return out

    def overlap_aabb(self, world, lo, hi):
        """As World.overlap_aabb, box i against world[i] (a scalar: all against that world) of the batch (mgf_batch_overlap_aabb_many):
        (offsets[n + 1], bodies) in CSR form, each list in ascending body index within the box's world."""
        return self.overlap_boxes(world, _boxes_from_corners(lo, hi))

    def overlap_boxes(self, world, boxes, cap=None):
        """overlap_aabb for mgf_aabb rows (c.xyz, r.xyz) as given; cap None sizes the output from a first call's count."""
        boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
        wd = _per_query(world, len(boxes))
        fn = load_library().mgf_batch_overlap_aabb_many
        return _overlap_lists(lambda *o: fn(self._h, wd.ctypes.data, boxes.ctypes.data, len(boxes), *o), len(boxes), cap)

    def _records(self, world, body):
        """(world, body) pairs as two contiguous int32 arrays of one length (a scalar world: every body of that world)"""
        bd = np.ascontiguousarray(np.atleast_1d(body), np.int32).reshape(-1)
        return _per_query(world, len(bd)), bd

    def get(self, world, body):
        """ConstrainedSet::get of body[i] of world[i] (mgf_batch_get_many): a BODY_GET_DTYPE array - linear, angular, x (= x + delta),
        restitution, friction, inv_mass, inv_moment (column-major), and the body's force and torque rows"""
        wd, bd = self._records(world, body)
        n = len(bd)
        vel, info = np.zeros((n, 6), np.float32), np.zeros((n, 15), np.float32)
        force, torque = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        _check(load_library().mgf_batch_get_many(self._h, wd.ctypes.data, bd.ctypes.data, n, vel.ctypes.data, info.ctypes.data,
                                                 force.ctypes.data, torque.ctypes.data))
        out = np.zeros(n, BODY_GET_DTYPE)
        out["linear"], out["angular"] = vel[:, 0:3], vel[:, 3:6]
        out["x"], out["restitution"], out["friction"], out["inv_mass"], out["inv_moment"] = info[:, 0:3], info[:, 3], info[:, 4], info[:, 5], info[:, 6:15]
        out["force"], out["torque"] = force, torque
        return out

    def set_velocities(self, world, body, linear, angular):
        """ConstrainedSet::set of body[i] of world[i] (mgf_batch_set_many), in array order: a body named twice keeps the last"""
        wd, bd = self._records(world, body)
        n = len(bd)
        vel = np.empty((n, 6), np.float32)
        vel[:, 0:3] = np.broadcast_to(np.asarray(linear, np.float32), (n, 3))
        vel[:, 3:6] = np.broadcast_to(np.asarray(angular, np.float32), (n, 3))
        _check(load_library().mgf_batch_set_many(self._h, wd.ctypes.data, bd.ctypes.data, n, vel.ctypes.data))

    def _rows3(self, a, n):
        return None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32), (n, 3)))

    def set_forces(self, world, body, force=None, torque=None):
        """RigidBodyVec.force / .torque of body[i] of world[i] (mgf_batch_set_forces), for every later tick until set again; None
        leaves that row as it is.  force is the stored one: world_force * mass."""
        wd, bd = self._records(world, body)
        f, t = self._rows3(force, len(bd)), self._rows3(torque, len(bd))
        _check(load_library().mgf_batch_set_forces(self._h, wd.ctypes.data, bd.ctypes.data, len(bd), _ptr(f), _ptr(t)))

    def apply_impulses(self, world, body, linear=None, angular=None):
        """v += linear * inv_mass, omega += inv_moment * angular on body[i] of world[i] (mgf_batch_apply_impulses); a body's records
        are applied in array order; None: zero"""
        wd, bd = self._records(world, body)
        a, b = self._rows3(linear, len(bd)), self._rows3(angular, len(bd))
        _check(load_library().mgf_batch_apply_impulses(self._h, wd.ctypes.data, bd.ctypes.data, len(bd), _ptr(a), _ptr(b)))

    def copy_worlds(self, dst_world, src, src_world):
        """world dst_world[i] of this batch becomes world src_world[i] of `src` (another batch of the context, or None / self: this
        one) on the device (mgf_batch_copy_worlds): bodies, colliders, the last tick's constraint list; a scalar src_world fans one
        world out.  The terrain assignment is not copied."""
        dw = np.ascontiguousarray(np.atleast_1d(dst_world), np.int32).reshape(-1)
        sw = _per_query(src_world, len(dw))
        s = self if src is None else src
        _check(load_library().mgf_batch_copy_worlds(self._h, dw.ctypes.data, s._h, sw.ctypes.data, len(dw)))

    # ---- the device-pointer calls: arguments are torch tensors on the context's device, or raw integer addresses -------------------------
    def body_index(self, world, body):
        """flat int32 indices of body[i] of world[i] (a scalar world: every body of that world), from the host's lengths: what the
        device-pointer calls name a body by - the order of state(None)"""
        lib = load_library()
        off = np.concatenate([[0], np.cumsum([lib.mgf_batch_len(self._h, k) for k in range(self.n_worlds)])]).astype(np.int64)
        wd, bd = self._records(world, body)
        if len(wd) and (wd.min() < 0 or wd.max() >= self.n_worlds):
            raise ValueError("world index out of range")
        if np.any(bd < 0) or np.any(bd >= (off[1:] - off[:-1])[wd]):
            raise ValueError("body index out of range")
        return (off[wd] + bd).astype(np.int32)

    def _dev_records(self, body, n):
        """(address of the flat indices or None, n) of a device-pointer call"""
        if body is None:
            return None, (len(self) if n is None else int(n))
        if n is None:
            if not hasattr(body, "data_ptr"):
                raise ValueError("n must be given with a raw address")
            n = int(body.numel())
        return _dev_arg(body, "int32", 1, int(n), "body"), int(n)

    def gather_state(self, body=None, x=None, q=None, v=None, omega=None, force=None, torque=None, n=None):
        """mgf_batch_gather_state_dev: x (= x + delta), q, v, omega, force, torque of the bodies `body` names (flat indices, a CUDA int32
        tensor; None: every body in order) into the CUDA float32 tensors given - n rows of 3, q of 4; None: not asked for.  Enqueued on
        the context's stream, not waited for."""
        bp, n = self._dev_records(body, n)
        p = [_dev_arg(a, "float32", 4 if k == 1 else 3, n, name)
             for k, (a, name) in enumerate(((x, "x"), (q, "q"), (v, "v"), (omega, "omega"), (force, "force"), (torque, "torque")))]
        _check(load_library().mgf_batch_gather_state_dev(self._h, bp, n, *p))

    def set_velocities_dev(self, body, linear, angular, n=None):
        """set_velocities with flat body indices and rows in device memory (mgf_batch_set_many_dev); both arrays are required"""
        if linear is None or angular is None:
            raise ValueError("linear and angular are both required")
        bp, n = self._dev_records(body, n)
        _check(load_library().mgf_batch_set_many_dev(self._h, bp, n, _dev_arg(linear, "float32", 3, n, "linear"), _dev_arg(angular, "float32", 3, n, "angular")))

    def set_forces_dev(self, body, force=None, torque=None, n=None):
        """set_forces with flat body indices and rows in device memory (mgf_batch_set_forces_dev); None leaves that row as it is"""
        bp, n = self._dev_records(body, n)
        _check(load_library().mgf_batch_set_forces_dev(self._h, bp, n, _dev_arg(force, "float32", 3, n, "force"), _dev_arg(torque, "float32", 3, n, "torque")))

    def apply_impulses_dev(self, body, linear=None, angular=None, n=None):
        """apply_impulses with flat body indices and rows in device memory (mgf_batch_apply_impulses_dev); None: zero"""
        bp, n = self._dev_records(body, n)
        _check(load_library().mgf_batch_apply_impulses_dev(self._h, bp, n, _dev_arg(linear, "float32", 3, n, "linear"), _dev_arg(angular, "float32", 3, n, "angular")))

    def body_contacts_dev(self, out, world=None):
        """body_contacts written straight into `out`: a CUDA float32 or int32 tensor of 6 words a body (BODY_CONTACTS_DTYPE's layout) for
        one world, or (world=None) the whole batch (mgf_batch_read_body_contacts_dev); not waited for"""
        w = -1 if world is None else int(world)
        n = max(load_library().mgf_batch_len(self._h, w), 0)
        words = "int32" if str(getattr(out, "dtype", "")) == "torch.int32" else "float32"
        _check(load_library().mgf_batch_read_body_contacts_dev(self._h, w, _dev_arg(out, words, 6, n, "out"), n))

    def copy_worlds_where(self, dst_world, src, src_world, mask):
        """copy_worlds for the pairs whose word of `mask` (a CUDA int32 tensor, one a pair) is not zero, read on the device
        (mgf_batch_copy_worlds_where); dst_world / src_world are host arrays as for copy_worlds.  Not waited for."""
        dw = np.ascontiguousarray(np.atleast_1d(dst_world), np.int32).reshape(-1)
        sw = _per_query(src_world, len(dw))
        s = self if src is None else src
        if mask is None:
            raise ValueError("mask is required")
        _check(load_library().mgf_batch_copy_worlds_where(self._h, dw.ctypes.data, s._h, sw.ctypes.data, len(dw), _dev_arg(mask, "int32", 1, len(dw), "mask")))

    def _dev_queries(self, world, q, q_cols, q_words, out, out_cols, ignore, n):
        """(world, queries, n, ignore, out) of a device-pointer query: addresses, None where the call takes NULL"""
        if q is None or out is None:
            raise ValueError("the queries and out are both required")
        if n is None:
            if not hasattr(q, "data_ptr") or q.dim() != 2:
                raise ValueError("n must be given with a raw address")
            n = int(q.shape[0])
        n = int(n)
        if world is None and n % self.n_worlds:
            raise ValueError("without world indices n is a multiple of the number of worlds")
        return (_dev_arg(world, "int32", 1, n, "world"), _dev_arg(q, q_words, q_cols, n, "queries"), n,
                _dev_arg(ignore, "int32", 1, n, "ignore"), _dev_arg(out, "int32", out_cols, n, "out"))

    def raycast_dev(self, world, parts, out, ignore=None, kinds=QUERY_ALL, n=None):
        """raycast with every array in device memory (mgf_batch_raycast_many_dev), enqueued on the context's stream and not waited for.
        world: CUDA int32 [n], the world of each particle - None: the fixed layout, n a multiple of n_worlds and particle i belongs
        to world i // (n // n_worlds).  parts: CUDA float32 [n, 7], a row (p.xyz, d.xyz, dt).  ignore: CUDA int32 [n] or None.
        out: CUDA int32 [n, 7], RAY_HIT_DTYPE's words - columns 0:3 are kind, index, part; view columns 3:7 (p.xyz, t) as float32
        (out[:, 3:].view(torch.float32)).  A particle whose world is out of range gets kind -1, the rest zero ("device_skipped")."""
        wp, qp, n, ip, op = self._dev_queries(world, parts, 7, "float32", out, 7, ignore, n)
        _check(load_library().mgf_batch_raycast_many_dev(self._h, wp, qp, n, ip, int(kinds), op))

    def sweep_dev(self, world, casts, out, ignore=None, kinds=QUERY_ALL, n=None):
        """sweep with every array in device memory (mgf_batch_sweep_many_dev), not waited for; world, ignore as for raycast_dev.
        casts: CUDA [n, 11], float32 or int32, MOVING_DTYPE's words (tag, p.xyz, d.xyz, r, delta.xyz): word 0 holds the tag's BITS - the
        integer 0 (sphere) or 1 (capsule), which in a float32 tensor is written through casts[:, 0].view(torch.int32).
        out: CUDA int32 [n, 13], SWEEP_HIT_DTYPE's words - columns 0:3 are kind, index, part; view columns 3:13 (a.xyz, b.xyz, n.xyz, t)
        as float32.  A cast whose world is out of range or whose tag is neither 0 nor 1 gets kind -1, the rest zero."""
        words = "int32" if str(getattr(casts, "dtype", "")) == "torch.int32" else "float32"
        wp, qp, n, ip, op = self._dev_queries(world, casts, 11, words, out, 13, ignore, n)
        _check(load_library().mgf_batch_sweep_many_dev(self._h, wp, qp, n, ip, int(kinds), op))

    # ---- body-mounted ray sensors: a rig set once, cast from the resident poses -----------------------------------------------------------
    def set_sensors(self, world, body=None, p=None, d=None, dt=float("inf"), ignore_self=True):
        """the batch's rig replaced (mgf_batch_set_sensors): sensor i is the ray from p[i] along d[i] for dt[i], all in the frame of
        body[i] of world[i]; ignore_self[i]: its own body is not a target.  Arrays, or scalars / single rows for all: the number of
        sensors is that of the longest argument.  No sensors (empty arrays) clears the rig.  Also takes a SENSOR_DTYPE array as
        `world` with every other argument None."""
        if isinstance(world, np.ndarray) and world.dtype == SENSOR_DTYPE:
            rig = np.ascontiguousarray(world.reshape(-1))
        else:
            rig = _rig_rows(SENSOR_DTYPE, world=world, body=body, p=p, d=d, dt=dt, flags=np.where(np.asarray(ignore_self, bool), SENSOR_IGNORE_SELF, 0))
        _check(load_library().mgf_batch_set_sensors(self._h, rig.ctypes.data if len(rig) else None, len(rig)))

    def sensor_count(self):
        return load_library().mgf_batch_sensor_count(self._h)

    def cast_sensors(self, kinds=QUERY_ALL, parts=False):
        """every sensor of the rig cast from its body's current pose (mgf_batch_cast_sensors): a RAY_HIT_DTYPE array in the rig's order,
        as raycast returns it; parts=True: (hits, particles) - the PARTICLE_DTYPE array of the rays in world coordinates"""
        n = max(self.sensor_count(), 0)
        out = np.zeros(n, RAY_HIT_DTYPE)
        pt = np.zeros(n, PARTICLE_DTYPE) if parts else None
        _check(load_library().mgf_batch_cast_sensors(self._h, int(kinds), out.ctypes.data, _ptr(pt), n))
        return (out, pt) if parts else out

    def cast_sensors_dev(self, out, kinds=QUERY_ALL, parts=None):
        """cast_sensors into device memory (mgf_batch_cast_sensors_dev), enqueued on the context's stream and not waited for.
        out: CUDA int32 [n, 7], RAY_HIT_DTYPE's words as raycast_dev writes them, n = sensor_count(); parts: CUDA float32 [n, 7] or
        None - a row (P.xyz, D.xyz, dt), the sensor's ray in world coordinates."""
        if out is None:
            raise ValueError("out is required")
        n = max(self.sensor_count(), 0)
        op, pp = _dev_arg(out, "int32", 7, n, "out"), _dev_arg(parts, "float32", 7, n, "parts")
        _check(load_library().mgf_batch_cast_sensors_dev(self._h, int(kinds), op, pp, n))

    # ---- body-mounted depth cameras: a rig set once, an image per camera from the resident poses ------------------------------------------
    def set_cameras(self, cams):
        """the batch's camera rig replaced (mgf_batch_set_cameras).  cams: a CAMERA_DTYPE array - camera i is fixed to body[i] of world[i]
        with its eye at p and the orientation r = (s, x, y, z) in the body's frame, looks along its own +z (+x right, +y up) with the half
        angles atan(tan_x), atan(tan_y), sees as far as `far` and has width x height pixels; flags: SENSOR_IGNORE_SELF or 0 - or a
        sequence of dicts with those keys (r defaults to the identity, far to inf, flags to SENSOR_IGNORE_SELF).  Empty: clears the rig."""
        if isinstance(cams, np.ndarray):
            if cams.dtype != CAMERA_DTYPE:
                raise ValueError(f"cams: a CAMERA_DTYPE array, not {cams.dtype}")
            rig = np.ascontiguousarray(cams.reshape(-1))
        else:
            cams = list(cams)
            rig = np.zeros(len(cams), CAMERA_DTYPE)
            rig["r"][:, 0], rig["far"], rig["flags"] = 1.0, np.inf, SENSOR_IGNORE_SELF
            for i, c in enumerate(cams):
                unknown = set(c) - set(CAMERA_DTYPE.names)
                if unknown:
                    raise ValueError(f"cams[{i}]: no such field: {sorted(unknown)}")
                for k, v in c.items():
                    rig[k][i] = v
        _check(load_library().mgf_batch_set_cameras(self._h, rig.ctypes.data if len(rig) else None, len(rig)))
        self._camera_shapes = [(int(h), int(w)) for h, w in zip(rig["height"], rig["width"])]

    def camera_count(self):
        return load_library().mgf_batch_camera_count(self._h)

    def camera_pixels(self):
        return load_library().mgf_batch_camera_pixels(self._h)

    def cast_cameras(self, kinds=QUERY_ALL, hits=False, parts=False):
        """every camera of the rig cast from its body's current pose (mgf_batch_cast_cameras): a list of [height, width] float32 depth
        images in the rig's order - the hit's t, or far where nothing is hit.  hits=True / parts=True: (images, hits[, parts]) - the
        flat RAY_HIT_DTYPE and PARTICLE_DTYPE arrays, camera by camera and row-major within a camera"""
        n = max(self.camera_pixels(), 0)
        depth = np.zeros(n, np.float32)
        out = np.zeros(n, RAY_HIT_DTYPE) if hits else None
        pt = np.zeros(n, PARTICLE_DTYPE) if parts else None
        _check(load_library().mgf_batch_cast_cameras(self._h, int(kinds), depth.ctypes.data, _ptr(out), _ptr(pt), n))
        images, at = [], 0
        for h, w in getattr(self, "_camera_shapes", []):
            images.append(depth[at:at + h * w].reshape(h, w))
            at += h * w
        res = (images,) + ((out,) if hits else ()) + ((pt,) if parts else ())
        return res if len(res) > 1 else images

    def cast_cameras_dev(self, depth=None, hits=None, parts=None, kinds=QUERY_ALL):
        """cast_cameras into device memory (mgf_batch_cast_cameras_dev), enqueued on the context's stream and not waited for.  With
        n = camera_pixels(): depth CUDA float32 [n], hits CUDA int32 [n, 7] (RAY_HIT_DTYPE's words as raycast_dev writes them), parts
        CUDA float32 [n, 7] (P.xyz, D.xyz, dt) - torch tensors or addresses; each may be None, but not depth and hits both."""
        if depth is None and hits is None:
            raise ValueError("depth or hits is required")
        n = max(self.camera_pixels(), 0)
        dp, op, pp = _dev_arg(depth, "float32", 1, n, "depth"), _dev_arg(hits, "int32", 7, n, "hits"), _dev_arg(parts, "float32", 7, n, "parts")
        _check(load_library().mgf_batch_cast_cameras_dev(self._h, int(kinds), dp, op, pp, n))

    # ---- box zones: a rig set once, the count and the first k bodies of every box from the resident poses --------------------------------
    def set_zones(self, world, body=None, p=(0.0, 0.0, 0.0), r=(0.0, 0.0, 0.0), ignore_self=None):
        """the batch's zone rig replaced (mgf_batch_set_zones): zone i is the axis-aligned box of half extents r[i] whose centre is
        p[i] in the frame of body[i] of world[i] - body None or -1: p[i] in the world; ignore_self[i]: its own body is not listed
        (None: wherever there is a body).  Arrays, or scalars / single rows for all: the number of zones is that of the longest
        argument.  No zones (empty arrays) clears the rig.  Also takes a ZONE_DTYPE array as `world` with every other argument left."""
        if isinstance(world, np.ndarray) and world.dtype == ZONE_DTYPE:
            rig = np.ascontiguousarray(world.reshape(-1))
        else:
            body = -1 if body is None else body
            flags = {} if ignore_self is None else dict(flags=np.where(np.asarray(ignore_self, bool), SENSOR_IGNORE_SELF, 0))
            rig = _rig_rows(ZONE_DTYPE, world=world, body=body, p=p, r=r, **flags)
            if ignore_self is None:
                rig["flags"] = np.where(rig["body"] >= 0, SENSOR_IGNORE_SELF, 0)
        _check(load_library().mgf_batch_set_zones(self._h, rig.ctypes.data if len(rig) else None, len(rig)))

    def zone_count(self):
        return load_library().mgf_batch_zone_count(self._h)

    def read_zones(self, k, boxes=False):
        """every zone of the rig from its body's current pose (mgf_batch_read_zones): (count[n], bodies[n, k]) int32 in the rig's
        order - count the bodies of the zone's world whose tight box overlaps the zone's, bodies the first k of them in ascending
        index, then -1; boxes=True: (count, bodies, boxes[n, 6]) - the boxes (c.xyz, r.xyz) as formed"""
        n, k = max(self.zone_count(), 0), int(k)
        out = np.zeros((n, 1 + max(k, 0)), np.int32)
        bx = np.zeros((n, 6), np.float32) if boxes else None
        _check(load_library().mgf_batch_read_zones(self._h, k, out.ctypes.data, _ptr(bx), n))
        return (out[:, 0], out[:, 1:]) + ((bx,) if boxes else ())

    def read_zones_dev(self, out, boxes=None, k=None):
        """read_zones into device memory (mgf_batch_read_zones_dev), enqueued on the context's stream and not waited for.
        out: CUDA int32 [n, 1 + k], n = zone_count() - column 0 the count, columns 1: the first k bodies, -1 behind them; k is
        out.shape[1] - 1 (a raw address: give k).  boxes: CUDA float32 [n, 6] or None - a row (c.xyz, r.xyz), the zone's box."""
        if out is None:
            raise ValueError("out is required")
        k = _record_k(out, k)
        n = max(self.zone_count(), 0)
        op, bp = _dev_arg(out, "int32", 1 + k, n, "out"), _dev_arg(boxes, "float32", 6, n, "boxes")
        _check(load_library().mgf_batch_read_zones_dev(self._h, k, op, bp, n))

    def overlap_first_dev(self, boxes, out, ignore=None, n=None, k=None):
        """the records of read_zones for boxes the caller computed on the device (mgf_batch_overlap_first_dev), not waited for.
        boxes: CUDA float32 [n, 6], a row (c.xyz, r.xyz); the fixed layout: n a multiple of n_worlds, box i against world
        i // (n // n_worlds).  out: CUDA int32 [n, 1 + k].  ignore: CUDA int32 [n] or None - a body of the box's world left out of its
        list.  Raw addresses: give n and k."""
        if boxes is None or out is None:
            raise ValueError("boxes and out are both required")
        if n is None:
            if not hasattr(boxes, "data_ptr") or boxes.dim() != 2:
                raise ValueError("n must be given with a raw address")
            n = int(boxes.shape[0])
        k = _record_k(out, k)
        n = int(n)
        if n % self.n_worlds:
            raise ValueError("n is a multiple of the number of worlds")
        bp, ip, op = _dev_arg(boxes, "float32", 6, n, "boxes"), _dev_arg(ignore, "int32", 1, n, "ignore"), _dev_arg(out, "int32", 1 + k, n, "out")
        _check(load_library().mgf_batch_overlap_first_dev(self._h, bp, n, ip, k, op))

    # ---- box zones, nearest first: the same rig, the k <= BATCH_ZONE_NEAREST_MAX_K nearest bodies of every box and their distances ---------
    def read_zones_nearest(self, k, dist2=False, boxes=False):
        """every zone of the rig, nearest first (mgf_batch_read_zones_nearest): (count[n], bodies[n, k]) int32 in the rig's order -
        count as read_zones', bodies the first k of the zone's list in ascending (d2, body index), d2 the squared distance of a body's
        tight box's centre from the zone's, then -1; dist2=True: then dist2[n, k] float32, +inf behind the listed ones; boxes=True:
        then boxes[n, 6] - the boxes (c.xyz, r.xyz) as formed"""
        n, k = max(self.zone_count(), 0), int(k)
        out = np.zeros((n, 1 + max(k, 0)), np.int32)
        d2 = np.zeros((n, max(k, 0)), np.float32) if dist2 else None
        bx = np.zeros((n, 6), np.float32) if boxes else None
        _check(load_library().mgf_batch_read_zones_nearest(self._h, k, out.ctypes.data, _ptr(d2), _ptr(bx), n))
        return (out[:, 0], out[:, 1:]) + ((d2,) if dist2 else ()) + ((bx,) if boxes else ())

    def read_zones_nearest_dev(self, out, dist2=None, boxes=None, k=None):
        """read_zones_nearest into device memory (mgf_batch_read_zones_nearest_dev), enqueued on the context's stream and not waited
        for.  out: CUDA int32 [n, 1 + k], n = zone_count() - column 0 the count, columns 1: the k nearest bodies, -1 behind them; k is
        out.shape[1] - 1 (a raw address: give k).  dist2: CUDA float32 [n, k] or None - their squared distances, +inf behind them.
        boxes: CUDA float32 [n, 6] or None - a row (c.xyz, r.xyz), the zone's box."""
        if out is None:
            raise ValueError("out is required")
        k = _record_k(out, k)
        n = max(self.zone_count(), 0)
        op, dp, bp = _dev_arg(out, "int32", 1 + k, n, "out"), _dev_arg(dist2, "float32", k, n, "dist2"), _dev_arg(boxes, "float32", 6, n, "boxes")
        _check(load_library().mgf_batch_read_zones_nearest_dev(self._h, k, op, dp, bp, n))

    def overlap_nearest_dev(self, boxes, out, dist2=None, ignore=None, n=None, k=None):
        """the records of read_zones_nearest for boxes the caller computed on the device (mgf_batch_overlap_nearest_dev), not waited
        for.  boxes: CUDA float32 [n, 6], a row (c.xyz, r.xyz); the fixed layout: n a multiple of n_worlds, box i against world
        i // (n // n_worlds).  out: CUDA int32 [n, 1 + k].  dist2: CUDA float32 [n, k] or None.  ignore: CUDA int32 [n] or None - a
        body of the box's world left out of its list.  Raw addresses: give n and k."""
        if boxes is None or out is None:
            raise ValueError("boxes and out are both required")
        if n is None:
            if not hasattr(boxes, "data_ptr") or boxes.dim() != 2:
                raise ValueError("n must be given with a raw address")
            n = int(boxes.shape[0])
        k = _record_k(out, k)
        n = int(n)
        if n % self.n_worlds:
            raise ValueError("n is a multiple of the number of worlds")
        bp, ip, op = _dev_arg(boxes, "float32", 6, n, "boxes"), _dev_arg(ignore, "int32", 1, n, "ignore"), _dev_arg(out, "int32", 1 + k, n, "out")
        dp = _dev_arg(dist2, "float32", k, n, "dist2")
        _check(load_library().mgf_batch_overlap_nearest_dev(self._h, bp, n, ip, k, op, dp))

    # ---- contact sensors: a rig set once, the last tick's constraint list folded per (body, partner) on the device ------------------------
    def set_touches(self, world, body=None, other=TOUCH_ANY, body_frame=False):
        """the batch's contact-sensor rig replaced (mgf_batch_set_touches): sensor i reports the records of world[i]'s last tick that
        name body[i] and whose partner passes other[i] - a body of that world, TOUCH_STATIC (terrain and obstacles), TOUCH_ANY_BODY or
        TOUCH_ANY; body_frame[i]: the report's three vectors in the frame of the body.  Arrays, or scalars for all: the number of
        sensors is that of the longest argument.  No sensors (empty arrays) clears the rig.  Also takes a TOUCH_DTYPE array as `world`
        with every other argument left."""
        if isinstance(world, np.ndarray) and world.dtype == TOUCH_DTYPE:
            rig = np.ascontiguousarray(world.reshape(-1))
        else:
            if body is None:
                raise ValueError("body is required")
            rig = _rig_rows(TOUCH_DTYPE, world=world, body=body, other=other, flags=np.where(np.asarray(body_frame, bool), TOUCH_BODY_FRAME, 0))
        _check(load_library().mgf_batch_set_touches(self._h, rig.ctypes.data if len(rig) else None, len(rig)))

    def touch_count(self):
        return load_library().mgf_batch_touch_count(self._h)

    def read_touches(self):
        """every sensor of the rig against the last tick's constraint list (mgf_batch_read_touches): a TOUCH_REPORT_DTYPE array in the
        rig's order - n_contacts, impulse and normal_impulse of the matching records folded in the body's chain order, and partner,
        record, push, strongest_impulse and arm of the strongest of them; nothing matched: n_contacts 0, partner TOUCH_NONE, record -1"""
        n = max(self.touch_count(), 0)
        out = np.zeros(n, TOUCH_REPORT_DTYPE)
        _check(load_library().mgf_batch_read_touches(self._h, out.ctypes.data if n else None, n))
        return out

    def read_touches_dev(self, out):
        """read_touches into device memory (mgf_batch_read_touches_dev), enqueued on the context's stream and not waited for.
        out: a CUDA tensor of int32 or float32 [n, 16], n = touch_count() - a row is TOUCH_REPORT_DTYPE's sixteen words - or a raw
        address."""
        if out is None:
            raise ValueError("out is required")
        n = max(self.touch_count(), 0)
        dtype = "float32" if str(getattr(out, "dtype", "")) == "torch.float32" else "int32"
        _check(load_library().mgf_batch_read_touches_dev(self._h, _dev_arg(out, dtype, 16, n, "out"), n))

    # ---- body-mounted feelers: a rig set once, spheres and capsules swept from the resident poses -----------------------------------------
    def set_feelers(self, world, body=None, tag=None, p=None, d=None, r=None, delta=None, ignore_self=True, world_delta=False, own_shape=False):
        """the batch's feeler rig replaced (mgf_batch_set_feelers): feeler i is the sphere (tag 0: centre p[i], radius r[i]) or capsule
        (tag 1: from p[i] along d[i], radius r[i]) in the frame of body[i] of world[i], swept by delta[i] - in the body's frame, or
        (world_delta[i]) in world coordinates; own_shape[i]: the cast is the body's own resident collider, and tag, p, d, r are not
        read (it needs ignore_self[i]); ignore_self[i]: its own body is not a target.  Arrays, or scalars / single rows for all: the
        number of feelers is that of the longest argument; an argument left None stays zero.  No feelers (empty arrays) clears the
        rig.  Also takes a FEELER_DTYPE array as `world` with every other argument None."""
        if isinstance(world, np.ndarray) and world.dtype == FEELER_DTYPE:
            rig = np.ascontiguousarray(world.reshape(-1))
        else:
            flags = (np.where(np.asarray(ignore_self, bool), FEELER_IGNORE_SELF, 0) | np.where(np.asarray(world_delta, bool), FEELER_WORLD_DELTA, 0)
                     | np.where(np.asarray(own_shape, bool), FEELER_OWN_SHAPE, 0))
            given = {k: v for k, v in dict(tag=tag, p=p, d=d, r=r, delta=delta).items() if v is not None}
            rig = _rig_rows(FEELER_DTYPE, world=world, body=body, flags=flags, **given)
        _check(load_library().mgf_batch_set_feelers(self._h, rig.ctypes.data if len(rig) else None, len(rig)))

    def feeler_count(self):
        return load_library().mgf_batch_feeler_count(self._h)

    def cast_feelers(self, kinds=QUERY_ALL, casts=False):
        """every feeler of the rig swept from its body's current pose (mgf_batch_cast_feelers): a SWEEP_HIT_DTYPE array in the rig's
        order, as sweep returns it; casts=True: (hits, casts) - the MOVING_DTYPE array of the casts in world coordinates"""
        n = max(self.feeler_count(), 0)
        out = np.zeros(n, SWEEP_HIT_DTYPE)
        cs = np.zeros(n, MOVING_DTYPE) if casts else None
        _check(load_library().mgf_batch_cast_feelers(self._h, int(kinds), out.ctypes.data, _ptr(cs), n))
        return (out, cs) if casts else out

    def cast_feelers_dev(self, out, kinds=QUERY_ALL, casts=None):
        """cast_feelers into device memory (mgf_batch_cast_feelers_dev), enqueued on the context's stream and not waited for.
        out: CUDA int32 [n, 13], SWEEP_HIT_DTYPE's words as sweep_dev writes them, n = feeler_count(); casts: CUDA [n, 11], float32 or
        int32, or None - MOVING_DTYPE's words (tag, p.xyz, d.xyz, r, delta.xyz) as sweep_dev reads them: word 0 holds the tag's BITS."""
        if out is None:
            raise ValueError("out is required")
        n = max(self.feeler_count(), 0)
        words = "int32" if str(getattr(casts, "dtype", "")) == "torch.int32" else "float32"
        op, cp = _dev_arg(out, "int32", 13, n, "out"), _dev_arg(casts, words, 11, n, "casts")
        _check(load_library().mgf_batch_cast_feelers_dev(self._h, int(kinds), op, cp, n))

    # ---- body-mounted actuators: a rig set once, wrenches formed from the resident poses and applied in one launch ------------------------
    def set_actuators(self, world, body=None, p=None, d=None, gain=1.0, lo=float("-inf"), hi=float("inf"), torque=False, world_dir=False):
        """the batch's actuator rig replaced (mgf_batch_set_actuators): actuator i acts on body[i] of world[i] along d[i] - in the
        body's frame, or (world_dir[i]) in world coordinates - at the arm p[i] in the body's frame, with gain[i] times its control
        clamped to [lo[i], hi[i]] (-inf / inf: no clamp); torque[i]: a pure couple about d[i], p is not read.  Arrays, or scalars /
        single rows for all: the number of actuators is that of the longest argument; p and d left None stay zero.  No actuators
        (empty arrays) clears the rig.  Also takes an ACTUATOR_DTYPE array as `world`, the other arguments not read."""
        if isinstance(world, np.ndarray) and world.dtype == ACTUATOR_DTYPE:
            rig = np.ascontiguousarray(world.reshape(-1))
        else:
            flags = np.where(np.asarray(torque, bool), ACTUATOR_TORQUE, 0) | np.where(np.asarray(world_dir, bool), ACTUATOR_WORLD_DIR, 0)
            given = {k: v for k, v in dict(p=p, d=d).items() if v is not None}
            rig = _rig_rows(ACTUATOR_DTYPE, world=world, body=body, flags=flags, gain=gain, lo=lo, hi=hi, **given)
        _check(load_library().mgf_batch_set_actuators(self._h, rig.ctypes.data if len(rig) else None, len(rig)))

    def actuator_count(self):
        return load_library().mgf_batch_actuator_count(self._h)

    def actuate(self, u, mode=ACTUATE_IMPULSE, wrenches=False):
        """the wrench of every actuator formed from its body's current q and its control u[i], and applied (mgf_batch_actuate):
        ACTUATE_IMPULSE as apply_impulses of those wrenches in the rig's order; ACTUATE_FORCE added to the force and torque rows, which
        accumulate from call to call and hold for every later tick.  u: one float an actuator (a scalar: for all).  wrenches=True:
        returns the float32 [n, 6] array of (L, A) in the rig's order."""
        n = max(self.actuator_count(), 0)
        uu = np.ascontiguousarray(np.broadcast_to(np.asarray(u, np.float32), (n,)))
        out = np.zeros((n, 6), np.float32) if wrenches else None
        _check(load_library().mgf_batch_actuate(self._h, uu.ctypes.data if n else None, n, int(mode), _ptr(out)))
        return out

    def actuate_dev(self, u, mode=ACTUATE_IMPULSE, wrenches_out=None):
        """actuate with the controls in device memory (mgf_batch_actuate_dev), enqueued on the context's stream and not waited for.
        u: CUDA float32 [n], n = actuator_count(); wrenches_out: CUDA float32 [n, 6] or None - (L, A) of every actuator."""
        if u is None:
            raise ValueError("u is required")
        n = max(self.actuator_count(), 0)
        up, wp = _dev_arg(u, "float32", 1, n, "u"), _dev_arg(wrenches_out, "float32", 6, n, "wrenches_out")
        _check(load_library().mgf_batch_actuate_dev(self._h, up, n, int(mode), wp))

    # ---- rollouts: T ticks under T rows of controls, a row of state traced behind every tick, in one step call ---------------------------
    def rollout(self, u, dt, iters, mode=ACTUATE_IMPULSE, body=None, trace=("x", "q", "v", "omega")):
        """T ticks as the loop actuate(u[t]) | step(dt, iters) | gather of `body` leaves the batch, with the step's one host wait
        (mgf_batch_rollout).  u: float32 [T, actuator_count()] (an int T where the rig is empty); body: flat indices (None: every
        body); trace: which of x (= x + delta), q, v, omega to return.  Returns a dict of float32 [T, m, 3 | 4] arrays by name and
        "stats", arr[t * n_worlds + k] = world k's tick t."""
        n = max(self.actuator_count(), 0)
        if isinstance(u, (int, np.integer)):
            if n:
                raise ValueError("u: a number of ticks stands for the controls of an empty rig only")
            uu = np.zeros((int(u), 0), np.float32)
        else:
            uu = np.ascontiguousarray(u, np.float32)
        if uu.ndim != 2 or uu.shape[1] != n:
            raise ValueError(f"u: {uu.shape} is not [T, {n}]")
        unknown = [k for k in trace if k not in ("x", "q", "v", "omega")]
        if unknown:
            raise ValueError(f"trace: {unknown[0]!r} is not one of x, q, v, omega")
        T = uu.shape[0]
        bb = None if body is None else np.ascontiguousarray(body, np.int32).reshape(-1)
        m = len(self) if bb is None else len(bb)
        out = {k: np.zeros((T, m, 4 if k == "q" else 3), np.float32) for k in ("x", "q", "v", "omega") if k in trace}
        arr = (StepStats * (T * self.n_worlds))()
        _check(load_library().mgf_batch_rollout(self._h, float(dt), int(iters), T, uu.ctypes.data if uu.size else None, n, int(mode),
                                                bb.ctypes.data if bb is not None and m else None, m,
                                                *[out[k].ctypes.data if k in out and out[k].size else None for k in ("x", "q", "v", "omega")], arr))
        out["stats"] = arr
        return out

    def rollout_dev(self, u, dt, iters, mode=ACTUATE_IMPULSE, body=None, x=None, q=None, v=None, omega=None):
        """rollout with the controls, the indices and the traces in device memory (mgf_batch_rollout_dev).  u: CUDA float32
        [T, actuator_count()] (an int T where the rig is empty); body: CUDA int32 [m] or None - every body; x, v, omega: CUDA float32
        [T, m, 3], q: [T, m, 4], None: not asked for.  Returns the statistics, arr[t * n_worlds + k] = world k's tick t; the traces
        are complete when the call returns (it waits as step does)."""
        if u is None:
            raise ValueError("u is required")
        n = max(self.actuator_count(), 0)
        if isinstance(u, (int, np.integer)):
            if n:
                raise ValueError("u: a number of ticks stands for the controls of an empty rig only")
            T, up = int(u), None
        else:
            if not hasattr(u, "data_ptr"):
                raise ValueError(f"u: a torch tensor on the GPU, not {type(u).__name__}")
            if u.dim() != 2 or u.shape[1] != n:
                raise ValueError(f"u: {tuple(u.shape)} is not [T, {n}]")
            T = int(u.shape[0])
            up = _dev_arg(u, "float32", n, T, "u")
        if body is None:
            bp, m = None, len(self)
        else:
            if not hasattr(body, "data_ptr"):
                raise ValueError(f"body: a torch tensor on the GPU, not {type(body).__name__}")
            m = int(body.numel())
            bp = _dev_arg(body, "int32", 1, m, "body")
        p = []
        for a, name, cols in ((x, "x", 3), (q, "q", 4), (v, "v", 3), (omega, "omega", 3)):
            if a is not None:
                if not hasattr(a, "data_ptr"):
                    raise ValueError(f"{name}: a torch tensor on the GPU, not {type(a).__name__}")
                if tuple(a.shape) != (T, m, cols):
                    raise ValueError(f"{name}: {tuple(a.shape)} is not [{T}, {m}, {cols}]")
            p.append(_dev_arg(a, "float32", m * cols, T, name))
        arr = (StepStats * (T * self.n_worlds))()
        _check(load_library().mgf_batch_rollout_dev(self._h, float(dt), int(iters), T, up, n, int(mode), bp, m, *p, arr))
        return arr

    # ---- rollout touch traces: the contact sensors' reports behind every tick of a rollout -------------------------------------------------
    def rollout_touches(self, u, dt, iters, mode=ACTUATE_IMPULSE, body=None, trace=("x", "q", "v", "omega"), short=False):
        """rollout, and row t of the contact sensors' reports behind tick t as well (mgf_batch_rollout_touches): the loop
        actuate(u[t]) | step(dt, iters) | gather of `body` | read_touches with the step's one host wait.  The arguments are rollout's;
        the result has one more entry, "touches": a TOUCH_REPORT_DTYPE array [T, touch_count()] in the rig's order, or (short) a
        TOUCH_SHORT_DTYPE one - n_contacts, partner, normal_impulse, strongest_impulse of those reports."""
        n = max(self.actuator_count(), 0)
        if isinstance(u, (int, np.integer)):
            if n:
                raise ValueError("u: a number of ticks stands for the controls of an empty rig only")
            uu = np.zeros((int(u), 0), np.float32)
        else:
            uu = np.ascontiguousarray(u, np.float32)
        if uu.ndim != 2 or uu.shape[1] != n:
            raise ValueError(f"u: {uu.shape} is not [T, {n}]")
        unknown = [k for k in trace if k not in ("x", "q", "v", "omega")]
        if unknown:
            raise ValueError(f"trace: {unknown[0]!r} is not one of x, q, v, omega")
        T = uu.shape[0]
        bb = None if body is None else np.ascontiguousarray(body, np.int32).reshape(-1)
        m = len(self) if bb is None else len(bb)
        out = {k: np.zeros((T, m, 4 if k == "q" else 3), np.float32) for k in ("x", "q", "v", "omega") if k in trace}
        nt = max(self.touch_count(), 0)
        touches = np.zeros((T, nt), TOUCH_SHORT_DTYPE if short else TOUCH_REPORT_DTYPE)
        arr = (StepStats * (T * self.n_worlds))()
        _check(load_library().mgf_batch_rollout_touches(self._h, float(dt), int(iters), T, uu.ctypes.data if uu.size else None, n, int(mode),
                                                        bb.ctypes.data if bb is not None and m else None, m,
                                                        *[out[k].ctypes.data if k in out and out[k].size else None for k in ("x", "q", "v", "omega")],
                                                        touches.ctypes.data if touches.size else None, nt,
                                                        ROLLOUT_TOUCH_SHORT if short else ROLLOUT_TOUCH_FULL, arr))
        out["touches"] = touches
        out["stats"] = arr
        return out

    def rollout_touches_dev(self, u, dt, iters, mode=ACTUATE_IMPULSE, body=None, x=None, q=None, v=None, omega=None, touches=None, short=False):
        """rollout_dev, and row t of the contact sensors' reports behind tick t as well (mgf_batch_rollout_touches_dev).  touches: a
        CUDA tensor of int32 or float32 [T, n, 16], n = touch_count() - an entry is TOUCH_REPORT_DTYPE's sixteen words - or (short)
        [T, n, 4], TOUCH_SHORT_DTYPE's four; a raw address; None: rollout_dev.  The other arguments and the result are rollout_dev's."""
        if u is None:
            raise ValueError("u is required")
        n = max(self.actuator_count(), 0)
        if isinstance(u, (int, np.integer)):
            if n:
                raise ValueError("u: a number of ticks stands for the controls of an empty rig only")
            T, up = int(u), None
        else:
            if not hasattr(u, "data_ptr"):
                raise ValueError(f"u: a torch tensor on the GPU, not {type(u).__name__}")
            if u.dim() != 2 or u.shape[1] != n:
                raise ValueError(f"u: {tuple(u.shape)} is not [T, {n}]")
            T = int(u.shape[0])
            up = _dev_arg(u, "float32", n, T, "u")
        if body is None:
            bp, m = None, len(self)
        else:
            if not hasattr(body, "data_ptr"):
                raise ValueError(f"body: a torch tensor on the GPU, not {type(body).__name__}")
            m = int(body.numel())
            bp = _dev_arg(body, "int32", 1, m, "body")
        p = []
        for a, name, cols in ((x, "x", 3), (q, "q", 4), (v, "v", 3), (omega, "omega", 3)):
            if a is not None:
                if not hasattr(a, "data_ptr"):
                    raise ValueError(f"{name}: a torch tensor on the GPU, not {type(a).__name__}")
                if tuple(a.shape) != (T, m, cols):
                    raise ValueError(f"{name}: {tuple(a.shape)} is not [{T}, {m}, {cols}]")
            p.append(_dev_arg(a, "float32", m * cols, T, name))
        nt, words = max(self.touch_count(), 0), 4 if short else 16
        if hasattr(touches, "data_ptr") and tuple(touches.shape) != (T, nt, words):
            raise ValueError(f"touches: {tuple(touches.shape)} is not [{T}, {nt}, {words}]")
        dtype = "float32" if str(getattr(touches, "dtype", "")) == "torch.float32" else "int32"
        tp = _dev_arg(touches, dtype, nt * words, T, "touches")
        arr = (StepStats * (T * self.n_worlds))()
        _check(load_library().mgf_batch_rollout_touches_dev(self._h, float(dt), int(iters), T, up, n, int(mode), bp, m, *p, tp, nt,
                                                            ROLLOUT_TOUCH_SHORT if short else ROLLOUT_TOUCH_FULL, arr))
        return arr

    # ---- rollout sensor traces: the ray sensors' answers behind every tick of a rollout ---------------------------------------------------
    def rollout_observe(self, u, dt, iters, mode=ACTUATE_IMPULSE, body=None, trace=("x", "q", "v", "omega"), touches=False, short=False, sensors=None,
                        kinds=QUERY_ALL):
        """rollout, and behind tick t row t of the contact sensors' reports (touches=True; short: rollout_touches') and / or row t of the
        ray sensors' answers (mgf_batch_rollout_observe): the loop actuate(u[t]) | step(dt, iters) | gather of `body` | read_touches |
        cast_sensors(kinds) with the step's one host wait.  sensors: "hit" - the result's "sensors" is a RAY_HIT_DTYPE array
        [T, sensor_count()] in the rig's order - or "depth" - a float32 [T, sensor_count()] array, a hit's t or the sensor's dt where
        nothing is hit - or None.  The other arguments and result entries are rollout_touches'."""
        if sensors not in (None, "hit", "depth"):
            raise ValueError(f"sensors: {sensors!r} is not one of 'hit', 'depth', None")
        n = max(self.actuator_count(), 0)
        if isinstance(u, (int, np.integer)):
            if n:
                raise ValueError("u: a number of ticks stands for the controls of an empty rig only")
            uu = np.zeros((int(u), 0), np.float32)
        else:
            uu = np.ascontiguousarray(u, np.float32)
        if uu.ndim != 2 or uu.shape[1] != n:
            raise ValueError(f"u: {uu.shape} is not [T, {n}]")
        unknown = [k for k in trace if k not in ("x", "q", "v", "omega")]
        if unknown:
            raise ValueError(f"trace: {unknown[0]!r} is not one of x, q, v, omega")
        T = uu.shape[0]
        bb = None if body is None else np.ascontiguousarray(body, np.int32).reshape(-1)
        m = len(self) if bb is None else len(bb)
        out = {k: np.zeros((T, m, 4 if k == "q" else 3), np.float32) for k in ("x", "q", "v", "omega") if k in trace}
        tr = ROLLOUT_TRACES()
        tr.touch_format = ROLLOUT_TOUCH_SHORT if short else ROLLOUT_TOUCH_FULL
        tr.sensor_format = ROLLOUT_SENSOR_DEPTH if sensors == "depth" else ROLLOUT_SENSOR_HIT
        tr.sensor_mask = int(kinds)
        if touches:
            nt = max(self.touch_count(), 0)
            out["touches"] = np.zeros((T, nt), TOUCH_SHORT_DTYPE if short else TOUCH_REPORT_DTYPE)
            tr.touch, tr.n_touch = (out["touches"].ctypes.data if out["touches"].size else None), nt
        if sensors is not None:
            ns = max(self.sensor_count(), 0)
            out["sensors"] = np.zeros((T, ns), np.float32 if sensors == "depth" else RAY_HIT_DTYPE)
            tr.sensor, tr.n_sensor = (out["sensors"].ctypes.data if out["sensors"].size else None), ns
        arr = (StepStats * (T * self.n_worlds))()
        _check(load_library().mgf_batch_rollout_observe(self._h, float(dt), int(iters), T, uu.ctypes.data if uu.size else None, n, int(mode),
                                                        bb.ctypes.data if bb is not None and m else None, m,
                                                        *[out[k].ctypes.data if k in out and out[k].size else None for k in ("x", "q", "v", "omega")],
                                                        C.byref(tr), arr))
        out["stats"] = arr
        return out

    def rollout_observe_dev(self, u, dt, iters, mode=ACTUATE_IMPULSE, body=None, x=None, q=None, v=None, omega=None, touches=None, short=False, sensors=None,
                            depth=False, kinds=QUERY_ALL):
        """rollout_touches_dev, and row t of the ray sensors' answers behind tick t as well (mgf_batch_rollout_observe_dev).  sensors: a
        CUDA tensor of int32 or float32 [T, n, 7], n = sensor_count() - an entry is RAY_HIT_DTYPE's seven words - or (depth) float32
        [T, n]; a raw address; None: rollout_touches_dev.  touches: rollout_touches_dev's, or None - no touch trace.  The other
        arguments and the result are rollout_dev's."""
        if u is None:
            raise ValueError("u is required")
        n = max(self.actuator_count(), 0)
        if isinstance(u, (int, np.integer)):
            if n:
                raise ValueError("u: a number of ticks stands for the controls of an empty rig only")
            T, up = int(u), None
        else:
            if not hasattr(u, "data_ptr"):
                raise ValueError(f"u: a torch tensor on the GPU, not {type(u).__name__}")
            if u.dim() != 2 or u.shape[1] != n:
                raise ValueError(f"u: {tuple(u.shape)} is not [T, {n}]")
            T = int(u.shape[0])
            up = _dev_arg(u, "float32", n, T, "u")
        if body is None:
            bp, m = None, len(self)
        else:
            if not hasattr(body, "data_ptr"):
                raise ValueError(f"body: a torch tensor on the GPU, not {type(body).__name__}")
            m = int(body.numel())
            bp = _dev_arg(body, "int32", 1, m, "body")
        p = []
        for a, name, cols in ((x, "x", 3), (q, "q", 4), (v, "v", 3), (omega, "omega", 3)):
            if a is not None:
                if not hasattr(a, "data_ptr"):
                    raise ValueError(f"{name}: a torch tensor on the GPU, not {type(a).__name__}")
                if tuple(a.shape) != (T, m, cols):
                    raise ValueError(f"{name}: {tuple(a.shape)} is not [{T}, {m}, {cols}]")
            p.append(_dev_arg(a, "float32", m * cols, T, name))
        tr = ROLLOUT_TRACES()
        tr.touch_format = ROLLOUT_TOUCH_SHORT if short else ROLLOUT_TOUCH_FULL
        tr.sensor_format = ROLLOUT_SENSOR_DEPTH if depth else ROLLOUT_SENSOR_HIT
        tr.sensor_mask = int(kinds)
        if touches is not None:
            nt, words = max(self.touch_count(), 0), 4 if short else 16
            if hasattr(touches, "data_ptr") and tuple(touches.shape) != (T, nt, words):
                raise ValueError(f"touches: {tuple(touches.shape)} is not [{T}, {nt}, {words}]")
            dtype = "float32" if str(getattr(touches, "dtype", "")) == "torch.float32" else "int32"
            tr.touch, tr.n_touch = _dev_arg(touches, dtype, nt * words, T, "touches"), nt
        if sensors is not None:
            ns = max(self.sensor_count(), 0)
            shape = (T, ns) if depth else (T, ns, 7)
            if hasattr(sensors, "data_ptr") and tuple(sensors.shape) != shape:
                raise ValueError(f"sensors: {tuple(sensors.shape)} is not {list(shape)}")
            dtype = "float32" if depth or str(getattr(sensors, "dtype", "")) == "torch.float32" else "int32"
            tr.sensor, tr.n_sensor = _dev_arg(sensors, dtype, ns * (1 if depth else 7), T, "sensors"), ns
        arr = (StepStats * (T * self.n_worlds))()
        _check(load_library().mgf_batch_rollout_observe_dev(self._h, float(dt), int(iters), T, up, n, int(mode), bp, m, *p, C.byref(tr), arr))
        return arr

    # ---- springs between bodies: a rig set once, impulses formed from the resident state and applied in two launches -----------------------
    def set_springs(self, world, body=None, other=-1, pa=None, pb=None, rest=0.0, k=0.0, c=0.0, lo=float("-inf"), hi=float("inf")):
        """the batch's spring rig replaced (mgf_batch_set_springs): spring i ties the arm pa[i] of body[i] - in the body's frame - to the
        arm pb[i] of other[i], both of world[i], or (other[i] = -1) to the point pb[i] of the world, with rest length rest[i], stiffness
        k[i], damping c[i] and the scalar force clamped to [lo[i], hi[i]] (-inf / inf: no clamp; a rope is lo = 0).  Arrays, or scalars
        / single rows for all: the number of springs is that of the longest argument; pa and pb left None stay zero.  No springs
        (empty arrays) clears the rig.  Also takes a SPRING_DTYPE array as `world`, the other arguments not read."""
        if isinstance(world, np.ndarray) and world.dtype == SPRING_DTYPE:
            rig = np.ascontiguousarray(world.reshape(-1))
        else:
            given = {key: v for key, v in dict(pa=pa, pb=pb).items() if v is not None}
            rig = _rig_rows(SPRING_DTYPE, world=world, body=body, other=other, rest=rest, k=k, c=c, lo=lo, hi=hi, **given)
        _check(load_library().mgf_batch_set_springs(self._h, rig.ctypes.data if len(rig) else None, len(rig)))

    def spring_count(self):
        return load_library().mgf_batch_spring_count(self._h)

    def apply_springs(self, h, wrenches=False):
        """the impulse of every spring over the time step h formed from the current state of its ends, and applied as apply_impulses of
        (body, L, A) and (other, Lb, Ab) in the rig's order (mgf_batch_apply_springs).  wrenches=True: returns the float32 [n, 12]
        array of (L, A, Lb, Ab) in the rig's order."""
        n = max(self.spring_count(), 0)
        out = np.zeros((n, 12), np.float32) if wrenches else None
        _check(load_library().mgf_batch_apply_springs(self._h, float(h), _ptr(out)))
        return out

    def apply_springs_dev(self, h, wrenches_out=None):
        """apply_springs enqueued on the context's stream and not waited for (mgf_batch_apply_springs_dev).  wrenches_out: CUDA
        float32 [n, 12], n = spring_count(), or None - (L, A, Lb, Ab) of every spring."""
        n = max(self.spring_count(), 0)
        _check(load_library().mgf_batch_apply_springs_dev(self._h, float(h), _dev_arg(wrenches_out, "float32", 12, n, "wrenches_out")))

    # ---- ball joints between bodies: a rig set once, sequential impulses over the resident velocities in one launch ------------------------
    def set_joints(self, world, body=None, other=-1, pa=None, pb=None, beta=0.0):
        """the batch's joint rig replaced (mgf_batch_set_joints): joint i ties the anchor pa[i] of body[i] - in the body's frame - to the
        anchor pb[i] of other[i], both of world[i], or (other[i] = -1) to the point pb[i] of the world; beta[i] in [0, 1] is the share
        of the gap removed per call.  Arrays, or scalars / single rows for all: the number of joints is that of the longest argument;
        pa and pb left None stay zero.  At most BATCH_MAX_WORLD_JOINTS joints a world.  No joints (empty arrays) clears the rig.  Also
        takes a JOINT_DTYPE array as `world`, the other arguments not read."""
        if isinstance(world, np.ndarray) and world.dtype == JOINT_DTYPE:
            rig = np.ascontiguousarray(world.reshape(-1))
        else:
            given = {key: v for key, v in dict(pa=pa, pb=pb).items() if v is not None}
            rig = _rig_rows(JOINT_DTYPE, world=world, body=body, other=other, beta=beta, **given)
        _check(load_library().mgf_batch_set_joints(self._h, rig.ctypes.data if len(rig) else None, len(rig)))

    def joint_count(self):
        return load_library().mgf_batch_joint_count(self._h)

    def solve_joints(self, h, iters, impulses=False):
        """`iters` sweeps of sequential impulses over every world's joints in the rig's order, from the current state of their ends:
        the velocities of every joint's two anchor points made to agree, beta / h of their gap added (mgf_batch_solve_joints).
        impulses=True: returns the float32 [n, 3] array of every joint's reaction over the call, in the rig's order."""
        n = max(self.joint_count(), 0)
        out = np.zeros((n, 3), np.float32) if impulses else None
        _check(load_library().mgf_batch_solve_joints(self._h, float(h), int(iters), _ptr(out)))
        return out

    def solve_joints_dev(self, h, iters, impulses_dev=None):
        """solve_joints enqueued on the context's stream and not waited for (mgf_batch_solve_joints_dev).  impulses_dev: CUDA
        float32 [n, 3], n = joint_count(), or None - every joint's reaction over the call."""
        n = max(self.joint_count(), 0)
        _check(load_library().mgf_batch_solve_joints_dev(self._h, float(h), int(iters), _dev_arg(impulses_dev, "float32", 3, n, "impulses_dev")))

    # ---- hinge joints between bodies: a point, two angular rows, a limit and a motor; the motors' targets a table of the handle's ------------
    def set_hinges(self, world, body=None, other=-1, pa=None, pb=None, ax=None, ua=None, bx=None, ub=None, beta=0.0, lo=0.0, hi=0.0, tmax=0.0,
                   limit=False, motor=False):
        """the batch's hinge rig replaced (mgf_batch_set_hinges): hinge i ties body[i] to other[i] of world[i] (other[i] = -1: to the
        world) at the anchors pa[i], pb[i] about the unit axes ax[i], bx[i], with the unit zero-angle references ua[i], ub[i] - each in
        its end's frame, as hinge_frames() returns them; beta[i] in [0, 1] is the share of the position error removed per call;
        limit[i]: the hinge angle is held to [lo[i], hi[i]] radians; motor[i]: the relative speed about the axis is driven to the
        target table's entry (set_hinge_targets), the torque capped at tmax[i] (np.inf: no cap).  cos and sin of (lo + hi) / 2 and of
        (hi - lo) / 2 are formed in float64 and rounded once.  Arrays, or scalars / single rows for all: the number of hinges is that
        of the longest argument.  At most BATCH_MAX_WORLD_HINGES hinges a world.  No hinges (empty arrays) clears the rig.  The target
        table becomes one row of zeros.  Also takes a HINGE_DTYPE array as `world`, the other arguments not read."""
        if isinstance(world, np.ndarray) and world.dtype == HINGE_DTYPE:
            rig = np.ascontiguousarray(world.reshape(-1))
        else:
            given = {key: v for key, v in dict(pa=pa, pb=pb, ax=ax, ua=ua, bx=bx, ub=ub).items() if v is not None}
            lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
            mid, half = (lo + hi) / 2, (hi - lo) / 2
            flags = np.asarray(limit, bool) * np.uint32(HINGE_LIMIT) + np.asarray(motor, bool) * np.uint32(HINGE_MOTOR)
            rig = _rig_rows(HINGE_DTYPE, world=world, body=body, other=other, beta=beta, tmax=tmax, flags=flags, cm=np.cos(mid), sm=np.sin(mid),
                            ch=np.cos(half), sh=np.sin(half), **given)
        _check(load_library().mgf_batch_set_hinges(self._h, rig.ctypes.data if len(rig) else None, len(rig)))

    def hinge_count(self):
        return load_library().mgf_batch_hinge_count(self._h)

    def set_hinge_targets(self, w):
        """the motors' target table replaced (mgf_batch_set_hinge_targets): w float32 [rows, hinge_count()] rad/s, or one row
        [hinge_count()].  solve_hinges names the row it reads; tick t of a rollout reads row min(t, rows - 1)."""
        n = max(self.hinge_count(), 0)
        w = np.ascontiguousarray(w, np.float32)
        if w.ndim == 1:
            w = w.reshape(1, -1)
        if w.ndim != 2 or w.shape[1] != n:
            raise ValueError(f"w: {w.shape} is not rows of {n} hinges")
        _check(load_library().mgf_batch_set_hinge_targets(self._h, w.ctypes.data if w.size else None, w.shape[0]))

    def set_hinge_targets_dev(self, w_dev, rows=None):
        """set_hinge_targets from device memory, enqueued on the context's stream and not waited for (mgf_batch_set_hinge_targets_dev).
        w_dev: CUDA float32 [rows, hinge_count()], or an integer address with `rows` given."""
        n = max(self.hinge_count(), 0)
        if rows is None:
            if not hasattr(w_dev, "data_ptr") or w_dev.dim() != 2:
                raise ValueError("w_dev: a tensor of rows of hinge_count() floats, or rows given with a raw address")
            rows = int(w_dev.shape[0])
        _check(load_library().mgf_batch_set_hinge_targets_dev(self._h, _dev_arg(w_dev, "float32", n, int(rows), "w_dev"), int(rows)))

    def solve_hinges(self, h, iters, row=0, impulses=False):
        """`iters` sweeps of sequential impulses over every world's hinges in the rig's order, from the current state of their ends:
        per hinge the motor, the limit, the two angular rows and the point (mgf_batch_solve_hinges); the motors' targets are row `row`
        of the table.  impulses=True: returns the float32 [n, 8] array (acc.x, acc.y, acc.z, a1, a2, al, am, 0) of every hinge - the
        point's reaction, the angular impulses, the limit's and the motor's over the call - in the rig's order."""
        n = max(self.hinge_count(), 0)
        out = np.zeros((n, 8), np.float32) if impulses else None
        _check(load_library().mgf_batch_solve_hinges(self._h, float(h), int(iters), int(row), _ptr(out)))
        return out

    def solve_hinges_dev(self, h, iters, row=0, impulses_dev=None):
        """solve_hinges enqueued on the context's stream and not waited for (mgf_batch_solve_hinges_dev).  impulses_dev: CUDA
        float32 [n, 8], n = hinge_count(), or None."""
        n = max(self.hinge_count(), 0)
        _check(load_library().mgf_batch_solve_hinges_dev(self._h, float(h), int(iters), int(row), _dev_arg(impulses_dev, "float32", 8, n, "impulses_dev")))

    # ---- the encoders of the hinges and the sliders, each call written once over a kind, _HINGE_ENC or _SLIDER_ENC; dev: the device form ------
    def _enc_call(self, kind, name, *args):
        _check(getattr(load_library(), "mgf_batch_" + name.format(kind[0]))(self._h, *args))

    def _enc_read(self, kind, out_dev=None, dev=False):
        n = max(getattr(self, kind[0] + "_count")(), 0)
        if dev:
            return self._enc_call(kind, "read_{}s_dev", _dev_arg(out_dev, "float32", 8, n, "out_dev"))
        out = np.zeros(n, kind[1])
        self._enc_call(kind, "read_{}s", out.ctypes.data if len(out) else None)
        return out

    def _enc_set_trace(self, kind, rows, full):
        self._enc_call(kind, "set_{}_trace", int(rows), kind[4] if full else kind[3])
        setattr(self, "_%s_trace_full" % kind[0], bool(full))

    def _enc_trace(self, kind, row0, rows, out_dev=None, dev=False):
        total = max(getattr(self, kind[0] + "_trace_rows")(), 0)
        rows = total - int(row0) if rows is None else int(rows)
        if row0 < 0 or rows < 0 or row0 + rows > total:
            raise ValueError(f"rows [{row0}, {row0 + rows}) are not rows of a table of {total}")
        n, full = max(getattr(self, kind[0] + "_count")(), 0), getattr(self, "_%s_trace_full" % kind[0], False)
        if dev:
            return self._enc_call(kind, "get_{}_trace_dev", _dev_arg(out_dev, "float32", 16 if full else 8, rows * n, "out_dev"), int(row0), rows)
        out = np.zeros((rows, n), kind[2] if full else kind[1])
        self._enc_call(kind, "get_{}_trace", out.ctypes.data if out.size else None, int(row0), rows)
        return out

    # ---- hinge encoders: angle, rate, limit side, gap and tilt of every hinge; a readings table every rollout fills, a row a tick ------------
    def read_hinges(self):
        """the reading of every hinge from the state as it stands (mgf_batch_read_hinges): a HINGE_READING_DTYPE array [hinge_count()]
        in the rig's order - c, sn (the angle is arctan2(sn, c): hinge_angles), rate, side (+1 / -1: the next solve's limit row is on,
        past hi / lo; 0: off), gap (the anchors' gap in the world) and tilt2 (the squared sine of the angle between the axes).  One
        launch, one download; the state is not touched."""
        return self._enc_read(_HINGE_ENC)

    def read_hinges_dev(self, out_dev):
        """read_hinges enqueued on the context's stream and not waited for (mgf_batch_read_hinges_dev).  out_dev: CUDA float32
        [hinge_count(), 8], or an integer address aligned to 16 bytes."""
        self._enc_read(_HINGE_ENC, out_dev, dev=True)

    def set_hinge_trace(self, rows, full=False):
        """the readings table made `rows` rows of hinge_count() entries of zeros (mgf_batch_set_hinge_trace): tick t < rows of every
        rollout form writes row t behind the tick, later ticks write nothing.  full=True: an entry also carries the eight impulse words
        of the tick's hinge solve (HINGE_TRACE_FULL_DTYPE; am / dt is the motor's torque).  rows = 0 frees the table: no trace, which
        is the default and what set_hinges leaves."""
        self._enc_set_trace(_HINGE_ENC, rows, full)

    def hinge_trace_rows(self):
        return load_library().mgf_batch_hinge_trace_rows(self._h)

    def hinge_trace(self, row0=0, rows=None):
        """rows [row0, row0 + rows) of the readings table (mgf_batch_get_hinge_trace; rows=None: to the table's end): an array
        [rows, hinge_count()] of HINGE_READING_DTYPE, or of HINGE_TRACE_FULL_DTYPE where the table was set with full=True.  One
        download, waited for."""
        return self._enc_trace(_HINGE_ENC, row0, rows)

    def hinge_trace_dev(self, out_dev, row0=0, rows=None):
        """hinge_trace as a device-to-device copy, enqueued on the context's stream and not waited for (mgf_batch_get_hinge_trace_dev).
        out_dev: CUDA float32 [rows * hinge_count(), 8] - 16 with full=True - or an integer address."""
        self._enc_trace(_HINGE_ENC, row0, rows, out_dev, dev=True)

    # ---- slider joints between bodies: three angular rows, two off-axis rows, a limit, a motor or a lock along the axis ---------------------
    def set_sliders(self, world, body=None, other=-1, pa=None, pb=None, ax=None, ua=None, bx=None, ub=None, beta=0.0, lo=0.0, hi=0.0, fmax=0.0,
                    limit=False, motor=False, lock=False):
        """the batch's slider rig replaced (mgf_batch_set_sliders): slider i ties body[i] to other[i] of world[i] (other[i] = -1: to the
        world) at the anchors pa[i], pb[i] along the unit axes ax[i], bx[i], with the unit references ua[i], ub[i] - each in its end's
        frame, as slider_frames() returns them; beta[i] in [0, 1] is the share of the position error removed per call; limit[i]: the
        travel along the axis is held to [lo[i], hi[i]]; motor[i]: the relative speed along the axis is driven to the target table's
        entry (set_slider_targets), the force capped at fmax[i] (np.inf: no cap); lock[i]: the travel is held at lo[i] - a weld -
        and neither limit[i] nor motor[i] may be set.  Arrays, or scalars / single rows for all: the number of sliders is that of the
        longest argument.  At most BATCH_MAX_WORLD_SLIDERS sliders a world.  No sliders (empty arrays) clears the rig.  The target
        table becomes one row of zeros.  Also takes a SLIDER_DTYPE array as `world`, the other arguments not read."""
        if isinstance(world, np.ndarray) and world.dtype == SLIDER_DTYPE:
            rig = np.ascontiguousarray(world.reshape(-1))
        else:
            given = {key: v for key, v in dict(pa=pa, pb=pb, ax=ax, ua=ua, bx=bx, ub=ub).items() if v is not None}
            flags = (np.asarray(limit, bool) * np.uint32(SLIDER_LIMIT) + np.asarray(motor, bool) * np.uint32(SLIDER_MOTOR) +
                     np.asarray(lock, bool) * np.uint32(SLIDER_LOCK))
            rig = _rig_rows(SLIDER_DTYPE, world=world, body=body, other=other, beta=beta, fmax=fmax, flags=flags, lo=lo, hi=hi, **given)
        _check(load_library().mgf_batch_set_sliders(self._h, rig.ctypes.data if len(rig) else None, len(rig)))

    def slider_count(self):
        return load_library().mgf_batch_slider_count(self._h)

    def set_slider_targets(self, w):
        """the motors' target table replaced (mgf_batch_set_slider_targets): w float32 [rows, slider_count()] length units a second, or
        one row [slider_count()].  solve_sliders names the row it reads; tick t of a rollout reads row min(t, rows - 1)."""
        n = max(self.slider_count(), 0)
        w = np.ascontiguousarray(w, np.float32)
        if w.ndim == 1:
            w = w.reshape(1, -1)
        if w.ndim != 2 or w.shape[1] != n:
            raise ValueError(f"w: {w.shape} is not rows of {n} sliders")
        _check(load_library().mgf_batch_set_slider_targets(self._h, w.ctypes.data if w.size else None, w.shape[0]))

    def set_slider_targets_dev(self, w_dev, rows=None):
        """set_slider_targets from device memory, enqueued on the context's stream and not waited for
        (mgf_batch_set_slider_targets_dev).  w_dev: CUDA float32 [rows, slider_count()], or an integer address with `rows` given."""
        n = max(self.slider_count(), 0)
        if rows is None:
            if not hasattr(w_dev, "data_ptr") or w_dev.dim() != 2:
                raise ValueError("w_dev: a tensor of rows of slider_count() floats, or rows given with a raw address")
            rows = int(w_dev.shape[0])
        _check(load_library().mgf_batch_set_slider_targets_dev(self._h, _dev_arg(w_dev, "float32", n, int(rows), "w_dev"), int(rows)))

    def solve_sliders(self, h, iters, row=0, impulses=False):
        """`iters` sweeps of sequential impulses over every world's sliders in the rig's order, from the current state of their ends:
        per slider the motor, the limit or the lock, the three angular rows and the two off-axis rows (mgf_batch_solve_sliders); the
        motors' targets are row `row` of the table.  impulses=True: returns the float32 [n, 8] array (p1, p2, al, am, aw.x, aw.y,
        aw.z, 0) of every slider - the off-axis impulses, the limit's or lock's, the motor's and the angular impulse over the call -
        in the rig's order."""
        n = max(self.slider_count(), 0)
        out = np.zeros((n, 8), np.float32) if impulses else None
        _check(load_library().mgf_batch_solve_sliders(self._h, float(h), int(iters), int(row), _ptr(out)))
        return out

    def solve_sliders_dev(self, h, iters, row=0, impulses_dev=None):
        """solve_sliders enqueued on the context's stream and not waited for (mgf_batch_solve_sliders_dev).  impulses_dev: CUDA
        float32 [n, 8], n = slider_count(), or None."""
        n = max(self.slider_count(), 0)
        _check(load_library().mgf_batch_solve_sliders_dev(self._h, float(h), int(iters), int(row), _dev_arg(impulses_dev, "float32", 8, n, "impulses_dev")))

    # ---- slider encoders: travel, rate, limit side, off-axis gap and frame error of every slider; a readings table every rollout fills -------
    def read_sliders(self):
        """the reading of every slider from the state as it stands (mgf_batch_read_sliders): a SLIDER_READING_DTYPE array
        [slider_count()] in the rig's order - d (the travel along the axis), rate (as the next solve's motor and axis rows see it), side
        (+1 / -1: the next solve's limit row is on, above hi / below lo; 2: locked; 0: off), off (the far anchor's distance from the
        axis along the two references) and e (the frames' error).  One launch, one download; the state is not touched."""
        return self._enc_read(_SLIDER_ENC)

    def read_sliders_dev(self, out_dev):
        """read_sliders enqueued on the context's stream and not waited for (mgf_batch_read_sliders_dev).  out_dev: CUDA float32
        [slider_count(), 8], or an integer address aligned to 16 bytes."""
        self._enc_read(_SLIDER_ENC, out_dev, dev=True)

    def set_slider_trace(self, rows, full=False):
        """the sliders' readings table made `rows` rows of slider_count() entries of zeros (mgf_batch_set_slider_trace): tick t < rows of
        every rollout form writes row t behind the tick, later ticks write nothing.  full=True: an entry also carries the eight impulse
        words of the tick's slider solve (SLIDER_TRACE_FULL_DTYPE; am / dt is the motor's force).  rows = 0 frees the table: no trace,
        which is the default and what set_sliders leaves."""
        self._enc_set_trace(_SLIDER_ENC, rows, full)

    def slider_trace_rows(self):
        return load_library().mgf_batch_slider_trace_rows(self._h)

    def slider_trace(self, row0=0, rows=None):
        """rows [row0, row0 + rows) of the sliders' readings table (mgf_batch_get_slider_trace; rows=None: to the table's end): an array
        [rows, slider_count()] of SLIDER_READING_DTYPE, or of SLIDER_TRACE_FULL_DTYPE where the table was set with full=True.  One
        download, waited for."""
        return self._enc_trace(_SLIDER_ENC, row0, rows)

    def slider_trace_dev(self, out_dev, row0=0, rows=None):
        """slider_trace as a device-to-device copy, enqueued on the context's stream and not waited for (mgf_batch_get_slider_trace_dev).
        out_dev: CUDA float32 [rows * slider_count(), 8] - 16 with full=True - or an integer address."""
        self._enc_trace(_SLIDER_ENC, row0, rows, out_dev, dev=True)

    def counter(self, name):
        v = C.c_int64()
        _check(load_library().mgf_batch_counter(self._h, name.encode(), C.byref(v)))
        return v.value

    def set_option(self, key, value):
        """mgf_batch_set_option: "cons_per_body" (1 .. 4096), or "part_queries" (0 | 1) - with 1 raycast, sweep, the sensors, feelers,
        box overlaps and zones of a batch that holds bodies of several components see their parts (a hit's `part`); the cameras do not"""
        _check(load_library().mgf_batch_set_option(self._h, key.encode(), int(value)))


def rccl_allow_override(allow=True):
    """Let the environment variable MGF_RCCL_LIB name the collectives library (before the first RCCL call of the process)."""
    _check(load_library().mgf_rccl_allow_override(1 if allow else 0))


def rccl_unique_id():
    """128 bytes from ncclGetUniqueId (rank 0 calls this and hands the bytes to the other ranks)."""
    buf = (C.c_ubyte * 128)()
    _check(load_library().mgf_rccl_unique_id(buf))
    return bytes(buf)


class Tiles:
    """This process's x-slab tiles of one scene behind mgf_tiles_* (the whole tile protocol under the C-ABI; mgf_amd.tiles is
    the same protocol in Python).  worlds[i] owns the slab x_ranges[i]; the tiles are first_tile .. of n_tiles_total."""

    def __init__(self, ctx, worlds, x_ranges, first_tile=0, n_tiles_total=None, halo=1.0, refresh_every=4, migrate=True):  # (refresh_every: tiles.DEFAULT_REFRESH_EVERY)
        self._ctx, self.worlds = ctx, list(worlds)
        n = len(self.worlds)
        total = n if n_tiles_total is None else int(n_tiles_total)
        big = 3.0e38
        lo = (C.c_float * n)(*[float(max(min(r[0], big), -big)) for r in x_ranges])
        hi = (C.c_float * n)(*[float(max(min(r[1], big), -big)) for r in x_ranges])
        hs = (C.c_void_p * n)(*[w._h for w in self.worlds])
        self._h = C.c_void_p()
        _check(load_library().mgf_tiles_create(ctx._h, n, hs, lo, hi, int(first_tile), total, float(halo), int(refresh_every),
                                               1 if migrate else 0, C.byref(self._h)))
        ctx._adopt(self)

    def __del__(self):
        if getattr(self, "_h", None):
            load_library().mgf_tiles_free(self._h)
            self._h = None

    def connect(self, unique_id, rank, n_ranks):
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        _check(load_library().mgf_tiles_connect(self._h, buf, int(rank), int(n_ranks)))

    def preflight(self):
        n = C.c_int32()
        _check(load_library().mgf_tiles_preflight(self._h, C.byref(n)))
        return n.value

    def step(self, dt, iters):
        arr = (StepStats * len(self.worlds))()
        _check(load_library().mgf_tiles_step(self._h, float(dt), int(iters), arr))
        return arr

    def migrated(self, tile, incoming=True):
        return load_library().mgf_tiles_migrated(self._h, int(tile), 1 if incoming else 0)

    def counter(self, key):
        """exchange_bytes_out / _in / _local, exchange_calls, exchange_ns, host_waits, ticks (mgf_tiles_counter)."""
        v = load_library().mgf_tiles_counter(self._h, key.encode())
        if v < 0:
            raise KeyError(key)
        return int(v)

    def set_option(self, key, value):
        _check(load_library().mgf_tiles_set_option(self._h, key.encode(), int(value)))
