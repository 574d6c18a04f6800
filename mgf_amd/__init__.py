"""mgf_amd — MI355X-native rigid-body step behind mgf's API.

Python host-side mirror of the reference's interface for the per-tick hot path
(RigidBodyVec / Solver / Contact / BVH<AABB> / Mesh / World::step), bound with ctypes to the
C-ABI in include/mgf_hip.h (mgf_amd/libmgf_hip.so, hand-written HIP kernels for gfx950).
There is no CPU fallback: importing works anywhere, but creating a Context without the built
library or without a GPU raises MgfError.
"""
from . import scenes  # noqa: F401
from ._capi import (MgfError, Context, Mesh, Bvh, World, WorldBatch, BATCH_MAX_BODIES, Solver, Tiles, rccl_unique_id, rccl_allow_override, Compound, contacts, contacts_batch, local_contacts_pair,  # noqa: F401
                    local_contacts_mesh, ray_capsule, intersections, particles, manifolds_from_contacts, inertia_tensor, geom_to_json, geom_from_json, default_params, lib_path, load_library,
                    COMPONENT_DTYPE, CONSTRAINT_DTYPE, MOVING_DTYPE, PARTICLE_DTYPE, INTERSECTION_DTYPE, CONTACT_DTYPE, LOCAL_CONTACT_DTYPE, MANIFOLD_DTYPE,
                    RAY_HIT_DTYPE, SWEEP_HIT_DTYPE, BODY_CONTACTS_DTYPE, BODY_GET_DTYPE, HIT_NONE, HIT_BODY, HIT_TERRAIN, HIT_OBSTACLE, QUERY_BODIES, QUERY_TERRAIN, QUERY_OBSTACLES, QUERY_ALL,
                    TOUCH_DTYPE, TOUCH_REPORT_DTYPE, TOUCH_STATIC, TOUCH_ANY_BODY, TOUCH_ANY, TOUCH_NONE, TOUCH_BODY_FRAME, BATCH_TOUCH_LAUNCHES,
                    FEELER_DTYPE, FEELER_IGNORE_SELF, FEELER_WORLD_DELTA, FEELER_OWN_SHAPE, BATCH_FEELER_LAUNCHES,
                    ACTUATOR_DTYPE, ACTUATOR_TORQUE, ACTUATOR_WORLD_DIR, ACTUATE_IMPULSE, ACTUATE_FORCE, BATCH_ACTUATOR_LAUNCHES,
                    BATCH_ROLLOUT_LAUNCHES_PER_TICK, SPRING_DTYPE, BATCH_SPRING_LAUNCHES, BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK,
                    JOINT_DTYPE, BATCH_JOINT_LAUNCHES, BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK, BATCH_MAX_WORLD_JOINTS,
                    HINGE_DTYPE, HINGE_LIMIT, HINGE_MOTOR, BATCH_HINGE_LAUNCHES, BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK, BATCH_MAX_WORLD_HINGES,
                    hinge_frames, HINGE_READING_DTYPE, HINGE_TRACE_FULL_DTYPE, HINGE_TRACE_READING, HINGE_TRACE_FULL, BATCH_HINGE_READ_LAUNCHES,
                    BATCH_ROLLOUT_HINGE_READ_LAUNCHES_PER_TICK, hinge_angles,
                    BatchSlider, SLIDER_DTYPE, SLIDER_LIMIT, SLIDER_MOTOR, SLIDER_LOCK, BATCH_SLIDER_LAUNCHES, BATCH_ROLLOUT_SLIDER_LAUNCHES_PER_TICK,
                    BATCH_MAX_WORLD_SLIDERS, slider_frames,
                    SLIDER_READING_DTYPE, SLIDER_TRACE_FULL_DTYPE, SLIDER_TRACE_READING, SLIDER_TRACE_FULL, BATCH_SLIDER_READ_LAUNCHES,
                    BATCH_ROLLOUT_SLIDER_READ_LAUNCHES_PER_TICK,
                    TOUCH_SHORT_DTYPE, ROLLOUT_TOUCH_FULL, ROLLOUT_TOUCH_SHORT, BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK,
                    ROLLOUT_TRACES, ROLLOUT_SENSOR_HIT, ROLLOUT_SENSOR_DEPTH, BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK)
