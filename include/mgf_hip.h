/*
 * mgf_hip.h — C-ABI of the MI355X-native rigid-body step behind mgf's API.
 *
 * The reference (maplant/mgf) is a pure-Rust crate with no FFI; its boundary for the
 * per-tick hot path is the public Rust API re-exported at src/lib.rs:117-150 and the
 * tick assembled in mgf_demo/world.rs:227-294.  Every entry point below cites the
 * reference item it replaces.  A Rust `extern "C"` shim binds these
 * one-to-one and turns non-OK statuses back into the panics the reference raises.
 *
 * Conventions
 *  - plain C, no torch types; opaque handles; (ptr,len) slices borrowed for the call;
 *    outputs into caller buffers with capacity + out-count (MGF_ERR_CAPACITY on overflow,
 *    out-count still reports the number required);
 *  - every call is synchronous: the context's HIP stream is drained before return, so
 *    Rust `&mut self` semantics hold; one handle = one thread at a time (Send, not Sync);
 *  - one mgf_ctx per GPU; all arithmetic is IEEE f32 with no FMA contraction, in the
 *    reference's operation order;
 *  - there is NO CPU fallback: without a HIP device every compute entry point returns
 *    MGF_ERR_HIP.
 */
#ifndef MGF_HIP_H
#define MGF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGF_API __attribute__((visibility("default")))

/* Rust panics on this path, mapped to status codes (SURVEY.md §8b "Errors"). */
typedef enum mgf_status {
  MGF_OK = 0,
  MGF_ERR_EMPTY = 1,        /* BVH::root on empty tree            bvh.rs:265          */
  MGF_ERR_NOT_OCCUPIED = 2, /* Pool index not occupied            pool.rs:111,160,170 */
  MGF_ERR_NOT_LEAF = 3,     /* BVH::get_leaf on a parent          bvh.rs:274          */
  MGF_ERR_STATIC_REF = 4,   /* RigidBodyRef::into() on Static     physics.rs:174      */
  MGF_ERR_SINGULAR = 5,     /* inertia tensor .invert().unwrap()  physics.rs:212      */
  MGF_ERR_INVALID = 6,      /* bad argument / radius assert       geom.rs:300,328     */
  MGF_ERR_CAPACITY = 7,     /* caller buffer too small                                 */
  MGF_ERR_HIP = 8,          /* HIP runtime failure or no device                        */
  MGF_ERR_OOM = 9
} mgf_status;

/* ---- POD mirrors of the reference's Copy types --------------------------------- */
typedef struct mgf_vec3 { float x, y, z; } mgf_vec3;               /* cgmath Vector3/Point3<f32> */
typedef struct mgf_quat { float s, x, y, z; } mgf_quat;            /* cgmath Quaternion<f32> {s, v} */
typedef struct mgf_aabb { mgf_vec3 c, r; } mgf_aabb;               /* geom.rs:257-260 centre + half extents */

/* Component (compound.rs:33): tag 0 = Sphere{c = p, r}; tag 1 = Capsule{a = p, d, r}. */
enum { MGF_SPHERE = 0, MGF_CAPSULE = 1, MGF_TRIANGLE = 2, MGF_RECTANGLE = 3, MGF_PLANE = 4,
       MGF_RAY = 5, MGF_SEGMENT = 6, MGF_AABB = 7 /* scene I/O only (mgf_geom_to_json): v = {p, d} / {a, b} / {c, r} */ };
typedef struct mgf_component { int32_t tag; mgf_vec3 p; mgf_vec3 d; float r; } mgf_component;
/* Moving<Component> (geom.rs:357): shape + per-step displacement. */
typedef struct mgf_moving_component { mgf_component shape; mgf_vec3 delta; } mgf_moving_component;

/* Generic shape operand for the single-shot narrowphase entry point:
 *   MGF_SPHERE   v = {c.xyz, r}            MGF_CAPSULE  v = {a.xyz, d.xyz, r}
 *   MGF_TRIANGLE v = {a.xyz, b.xyz, c.xyz} MGF_PLANE    v = {n.xyz, d}
 * (MGF_RECTANGLE is not on the hot path: MGF_ERR_INVALID.) */
typedef struct mgf_shape { int32_t kind; float v[12]; } mgf_shape;

typedef struct mgf_contact { mgf_vec3 a, b, n; float t; } mgf_contact;                 /* collision.rs:431-442 */
typedef struct mgf_local_contact { mgf_vec3 local_a, local_b; mgf_contact global; } mgf_local_contact; /* :1410-1419 */

/* RigidBodyRef (physics.rs:158-162): tag 0 Dynamic(index), tag 1 Static{center, friction}. */
typedef struct mgf_body_ref { int32_t tag; uint32_t index; mgf_vec3 center; float friction; } mgf_body_ref;
typedef struct mgf_velocity { mgf_vec3 linear, angular; } mgf_velocity;                /* physics.rs:133-137 */
typedef struct mgf_rigid_body_info {                                                   /* physics.rs:124-130 */
  mgf_vec3 x; float restitution, friction, inv_mass; float inv_moment[9]; /* column-major */
} mgf_rigid_body_info;

/* Compile-time trait constants of the reference, as run-time parameters. */
typedef struct mgf_params {
  float baumgarte;               /* solver.rs:278   0.2  */
  float penetration_slop;        /* solver.rs:277   0.05 */
  float persistent_threshold_sq; /* manifold.rs:38  0.5  */
  float collision_epsilon;       /* geom.rs:27      1e-6 (informational: baked into the kernels) */
  float fat_margin;              /* world.rs:181    0.25 */
} mgf_params;

/* One contact constraint as the solver holds it (solver.rs:82-93, 256-262), flattened for
 * the single-contact manifolds this path produces.  Read-back/debug and bulk-insert format. */
typedef struct mgf_constraint {
  int32_t a, b;                 /* body indices; b = -1 for RigidBodyRef::Static */
  int32_t n_contacts;
  mgf_vec3 normal, t0, t1, ra, rb;
  float bias, normal_mass, tangent_mass0, tangent_mass1, normal_impulse, friction;
} mgf_constraint;

typedef struct mgf_step_stats {
  uint64_t n_bodies;
  uint64_t n_constraints;          /* ContactConstraints handed to the Solver this tick            */
  uint64_t n_terrain_constraints;  /* of which body-vs-Mesh (one per terrain contact, world.rs:243) */
  uint64_t n_pair_candidates;      /* broadphase hits (j < i, tight_i overlaps fat_j)               */
  /* (LIMIT: counted from the bodies' own boxes.  The reference reaches a leaf of its tree only through the leaf's ancestors (bvh.rs:283-310),
   * whose boxes are (upper + lower) / 2 rounded to f32: about 1e5 from the origin, where an ulp is 1/128, such a box can miss its child by that
   * ulp and the reference then skips a pair whose boxes touch exactly.  The count - and the pair, which is tested for contacts here - can exceed the
   * reference's by such pairs; up to coordinates of 1e4 no test has seen one.  tests/contact_corpus.py: LeafRecount.) */
  uint64_t n_terrain_candidates;   /* mesh-BVH face hits                                            */
  uint64_t n_refits;               /* bodies whose swept AABB left their fat AABB (world.rs:235)    */
  uint32_t n_levels;               /* depth of the order-preserving dependency DAG                  */
  uint32_t iters;
  float ms_integrate, ms_broadphase, ms_narrowphase, ms_setup, ms_solve, ms_total; /* HIP-event times of the phases: 0 unless option "phase_timing" is on (each event is a barrier packet: ~50 us of an idle GPU per tick together) */
  uint64_t solver_kernel_launches; /* number of solver kernel launches this tick     */
  float ms_solver_kernels;         /* sum of their HIP-event durations (0 if not timed) */
  uint64_t n_ghost_constraints;    /* of n_constraints: those whose obj_a is a ghost body of a neighbouring tile - a constraint across
                                      a tile face exists on both tiles, on each with the other tile's body as obj_a (0 without tiles) */
} mgf_step_stats;

/* Particle (geom.rs:802-855): a Ray { p, d } has dt = INFINITY; a Segment { a, b } is p = a, d = b - a, dt = 1. */
typedef struct { mgf_vec3 p; mgf_vec3 d; float dt; } mgf_particle;
/* Intersection collision.rs:151-158 */
typedef struct { mgf_vec3 p; float t; } mgf_intersection;

/* Manifold manifold.rs:112-118: time, normal (the UN-renormalised mean of the kept contacts' normals; NaN for an empty
 * group, as in the reference), tangent_vector[2] = compute_basis(normal), the kept (local_a, local_b) pairs. */
#define MGF_MANIFOLD_CAP 8
typedef struct {
  float time; mgf_vec3 normal; mgf_vec3 tangent[2]; int32_t n_contacts;
  mgf_vec3 local_a[MGF_MANIFOLD_CAP]; mgf_vec3 local_b[MGF_MANIFOLD_CAP];
} mgf_manifold;

typedef struct mgf_ctx mgf_ctx;
typedef struct mgf_mesh mgf_mesh;
typedef struct mgf_bvh mgf_bvh;
typedef struct mgf_world mgf_world;
typedef struct mgf_compound mgf_compound;
typedef struct mgf_solver mgf_solver;
typedef struct mgf_tiles mgf_tiles;
typedef struct mgf_batch mgf_batch;

/* ---- context ---------------------------------------------------------------------- */
MGF_API mgf_status mgf_ctx_create(int device, mgf_ctx** out);
/* Waits for the context's stream and drops the creator's reference.  Handles made from the context (worlds, meshes, trees, compounds, tile sets)
 * hold references of their own: those still alive keep the struct and its streams until they are freed, in whatever order a garbage collector
 * or a scope frees them; every other call on such a handle fails with MGF_ERR_INVALID ("the context was destroyed"). */
MGF_API void mgf_ctx_destroy(mgf_ctx* ctx);
/* Enqueue all work of this context on a caller-owned hipStream_t (e.g. the stream the caller's RCCL
 * transfers are ordered on) instead of the context's own stream.  The caller keeps ownership. */
MGF_API mgf_status mgf_ctx_set_stream(mgf_ctx* ctx, void* hip_stream);
/* Waits for the context's stream (its own, or the caller's after mgf_ctx_set_stream) and for nothing else on the device: how a caller
 * who shares no stream with the library waits for the calls that return without waiting (the mgf_batch_*_dev calls). */
MGF_API mgf_status mgf_ctx_synchronize(mgf_ctx* ctx);
MGF_API const char* mgf_last_error(void);        /* thread-local message for the last non-OK status */
MGF_API mgf_params mgf_default_params(void);     /* DefaultContactConstraintParams / DefaultPruningParams */
MGF_API const char* mgf_version(void);
/* The device-wide exclusive scan the tick uses for its list offsets (csrc/prims.hip: rocPRIM), on host arrays:
 * out[i] = sum of in[0..i).  Exposed so that the primitive can be tested on its own. */
MGF_API mgf_status mgf_exclusive_scan_u32(mgf_ctx* ctx, const uint32_t* in, int64_t n, uint32_t* out);

/* ---- single-shot narrowphase (unit parity; runs the same device functions as the step) ---
 * Contacts::contacts (collision.rs:471-482) for `a` [moving by vel_a] vs `b` [moving by vel_b];
 * NULL velocity = static operand.  Dispatch follows the reference's trait resolution
 * (collision.rs:484-494, 521-1401).  *count = number of contacts emitted. */
MGF_API mgf_status mgf_contacts(mgf_ctx* ctx, const mgf_shape* a, const mgf_vec3* vel_a, const mgf_shape* b,
                                const mgf_vec3* vel_b, mgf_contact* out, int32_t cap, int32_t* count);
/* Batched form: n independent (a, vel_a, b, vel_b) problems; has_vel bit0 = a moving, bit1 = b moving.
 * out holds 2 slots per problem (no pair on this path emits more), counts[n]. */
MGF_API mgf_status mgf_contacts_batch(mgf_ctx* ctx, int64_t n, const mgf_shape* a, const mgf_vec3* vel_a,
                                      const mgf_shape* b, const mgf_vec3* vel_b, const uint8_t* has_vel,
                                      mgf_contact* out, int32_t* counts);
/* (r06, no reference counterpart: a test entry point) n independent (moving component, triangle) problems - tris: three vertices each - through the
 * cheap conservative reject the tick's front end runs ahead of the body-triangle tests AND through those tests (Contacts<Moving<Component>> for
 * Triangle, collision.rs:610-1086, compound.rs:180-190): far[i] = 1 if the reject drops the problem, counts[i] = contacts the tests report.  A
 * problem with far[i] = 1 and counts[i] > 0 would be a contact the tick loses; tests/test_gpu_tri_reject.py looks for one in millions. */
MGF_API mgf_status mgf_tri_reject_batch(mgf_ctx* ctx, int64_t n, const mgf_moving_component* bodies, const mgf_vec3* tris,
                                        uint8_t* far, int32_t* counts);
/* LocalContacts<Moving<Component>> for Moving<Component> (compound.rs:192-207). */
MGF_API mgf_status mgf_local_contacts_pair(mgf_ctx* ctx, const mgf_moving_component* a, const mgf_moving_component* b,
                                           mgf_local_contact* out, int32_t cap, int32_t* count);
/* Intersects<Capsule>/<Sphere> for Ray (collision.rs:249-359); *hit = 0/1. */
MGF_API mgf_status mgf_ray_capsule(mgf_ctx* ctx, const mgf_vec3* p, const mgf_vec3* d, const mgf_shape* capsule,
                                   mgf_vec3* ip, float* t, int32_t* hit);
/* Inertia::tensor (physics.rs:26-93), column-major 3x3. */
MGF_API mgf_status mgf_inertia_tensor(const mgf_component* c, float mass, float out9[9]);

/* ---- Mesh (mesh.rs:32-73, geom.rs:459): static triangle soup + BVH<AABB,usize> over faces ---- */
MGF_API mgf_status mgf_mesh_new(mgf_ctx* ctx, mgf_mesh** out);                        /* Mesh::new         mesh.rs:40 */
MGF_API void mgf_mesh_free(mgf_mesh* m);
MGF_API mgf_status mgf_mesh_push_vert(mgf_mesh* m, mgf_vec3 p, uint64_t* id);         /* Mesh::push_vert   mesh.rs:58 */
MGF_API mgf_status mgf_mesh_push_face(mgf_mesh* m, uint64_t a, uint64_t b, uint64_t c, uint64_t* id); /* mesh.rs:64 */
MGF_API mgf_status mgf_mesh_set_pos(mgf_mesh* m, mgf_vec3 p);                         /* Shape::set_pos    geom.rs:459 */
MGF_API mgf_status mgf_mesh_build(mgf_mesh* m, const mgf_vec3* verts, int64_t nverts, const uint32_t* faces,
                                  int64_t nfaces);                                    /* bulk push_vert/push_face */
/* LocalContacts<Mesh> for Moving<Component> (collision.rs:1490-1506 over mesh.rs:115-139),
 * contacts in mesh-BVH DFS order. */
MGF_API mgf_status mgf_local_contacts_mesh(mgf_ctx* ctx, const mgf_moving_component* body, const mgf_mesh* mesh,
                                           mgf_local_contact* out, int32_t cap, int32_t* count);

/* ---- BVH<AABB, usize> (bvh.rs:30-310): reference-faithful dynamic tree (insert/remove/balance
 * are inherently sequential and run on the host); queries traverse the uploaded tree on the GPU
 * with the reference's stack discipline, so hit order equals the reference's DFS order. ---- */
MGF_API mgf_status mgf_bvh_new(mgf_ctx* ctx, mgf_bvh** out);                          /* BVH::new            bvh.rs:88  */
MGF_API mgf_status mgf_bvh_with_capacity(mgf_ctx* ctx, uint64_t cap, mgf_bvh** out);  /* BVH::with_capacity  bvh.rs:96  */
MGF_API void mgf_bvh_free(mgf_bvh* b);
MGF_API int32_t mgf_bvh_empty(const mgf_bvh* b);                                      /* BVH::empty          bvh.rs:104 */
MGF_API mgf_status mgf_bvh_clear(mgf_bvh* b);                                         /* BVH::clear          bvh.rs:109 */
MGF_API mgf_status mgf_bvh_insert(mgf_bvh* b, const mgf_aabb* key, uint64_t val, uint64_t* id); /* bvh.rs:125 */
MGF_API mgf_status mgf_bvh_remove(mgf_bvh* b, uint64_t id);                           /* BVH::remove         bvh.rs:220 */
MGF_API mgf_status mgf_bvh_root(const mgf_bvh* b, uint64_t* id);                      /* BVH::root           bvh.rs:263 */
MGF_API mgf_status mgf_bvh_get_leaf(const mgf_bvh* b, uint64_t id, uint64_t* val);    /* BVH::get_leaf       bvh.rs:270 */
MGF_API mgf_status mgf_bvh_bounds(const mgf_bvh* b, uint64_t id, mgf_aabb* out);      /* Index<usize>        bvh.rs:483 */
typedef void (*mgf_bvh_hit_fn)(const uint64_t* val, void* user);
MGF_API mgf_status mgf_bvh_query(mgf_bvh* b, const mgf_aabb* arg, mgf_bvh_hit_fn cb, void* user); /* bvh.rs:283 */
/* Bulk query: n AABBs; hits of query q are out_vals[out_offsets[q] .. out_offsets[q+1]) in DFS order. */
MGF_API mgf_status mgf_bvh_query_many(mgf_bvh* b, const mgf_aabb* args, int64_t n, uint64_t* out_offsets /* n+1 */,
                                      uint64_t* out_vals, int64_t cap, int64_t* total);
/* BVH::raytrace (bvh.rs:345-369): every leaf whose bounds the particle intersects, with that intersection, in the
 * reference's visiting order; _many is the bulk form (CSR offsets per particle). */
typedef void (*mgf_bvh_ray_fn)(const uint64_t* value, const mgf_intersection* inter, void* user);
MGF_API mgf_status mgf_bvh_raytrace(mgf_bvh* b, const mgf_particle* arg, mgf_bvh_ray_fn cb, void* user);
MGF_API mgf_status mgf_bvh_raytrace_many(mgf_bvh* b, const mgf_particle* args, int64_t n, uint64_t* out_offsets, uint64_t* out_vals,
                                         mgf_intersection* out_inter, int64_t cap, int64_t* total);
/* Intersects<Sphere | Capsule | Triangle | Plane> (shapes != NULL) or Intersects<AABB> (boxes != NULL) for n
 * particle/target pairs (collision.rs:169-373); hit[i] = 1 and out[i] filled, or hit[i] = 0. */
MGF_API mgf_status mgf_intersections_batch(mgf_ctx* ctx, int64_t n, const mgf_particle* parts, const mgf_shape* shapes,
                                           const mgf_aabb* boxes, mgf_intersection* out, int32_t* hit);

/* ---- World: RigidBodyVec + Solver + broadphase + terrain, resident in HBM for the whole tick.
 * Replaces mgf_demo/world.rs: World::add_body :178-184 and World::step :227-294, built on
 * RigidBodyVec (physics.rs:141-315), ContactPruner/Manifold (manifold.rs), ContactConstraint and
 * Solver (solver.rs).  Constraint insertion order: body i ascending; for each i the terrain
 * contacts in mesh-BVH DFS order, then partners j < i ascending (DESIGN.md "constraint order"). ---- */
MGF_API mgf_status mgf_world_new(mgf_ctx* ctx, const mgf_params* params, mgf_world** out);
MGF_API void mgf_world_free(mgf_world* w);
MGF_API mgf_status mgf_world_set_terrain(mgf_world* w, const mgf_mesh* mesh);         /* copies; World.terrain */
/* A static Compound (compound.rs:230-352) as an obstacle of the world beside the Mesh (copied; its pose as set when it is added).
 * Every tick each owned body's parts go through Compound::contacts (:334-352) after the body's terrain contacts - obstacles in the
 * order they were added, the body's parts in order - and every contact becomes a constraint against
 * Static{center: the compound's displacement (Shape::center, :289-291), friction: 0}: world.rs:243-251 with the compound in the Mesh's
 * place (the reference's demo world holds a Mesh only; the oracle states the definition, World::obstacles).  At most 256 obstacles of at most 2^18 components each. */
MGF_API mgf_status mgf_world_add_obstacle(mgf_world* w, const mgf_compound* c);
/* World::add_body / RigidBodyVec::add_body (physics.rs:200-218), bulk; MGF_ERR_SINGULAR as the unwrap. */
MGF_API mgf_status mgf_world_add_bodies(mgf_world* w, const mgf_component* comps, int64_t n, const float* mass,
                                        const float* restitution, const float* friction, const mgf_vec3* world_force,
                                        uint64_t* first_id);
/* Bodies of several components (BASELINE config 5).  NOT in the reference - physics.rs:200 takes one Component - so the
 * definition is this build's (oracle: RigidBodyVec::add_compound_body): body b is made of comps[offsets[b] ..
 * offsets[b + 1]) (1..32 components, world coordinates at creation) with masses comp_mass[..]; mass = sum, x = centre of
 * mass, q = identity, inertia = sum of the components' tensors about the centre of mass (the reference's Inertia,
 * physics.rs:30-93); the parts are fixed in the body frame and rebuilt from (x, q) every tick like a single collider
 * (physics.rs:243-251).  Contacts: every pair of parts in order, the first body's outer (Contacts, compound.rs:180-190), local points
 * relative to the bodies' centres, ContactPruner + Manifold::from(pruner) (manifold.rs:72-148) - up to 16 contacts per pair of bodies,
 * each a consecutive single-contact constraint record with the manifold's normal (equivalent to solver.rs:219-248).
 * Bodies of up to 4 components keep their parts in four slots per body; ghost and migrant records carry those four, so such bodies cross
 * tiles like the others (kind bits 2 and 3 of "body_kinds").  Bodies of 5..32 components (r06) keep theirs in a pool of the
 * world; a wave takes a candidate pair of bodies and its lanes the part pairs (the reference's Compound, compound.rs:232-352, a STATIC
 * shape, walks a BVH over its components instead - one CPU thread's way of skipping distant parts).
 * LIMITS: a body of more than 32 components (or of none) is refused with MGF_ERR_INVALID and nothing is added; bodies of more than 4
 * components are refused in tile sets (MGF_ERR_INVALID: the tile records carry four part slots); a tick in which two bodies meet in more
 * than 64 part pairs, or in a manifold of more than 16 contacts, fails with MGF_ERR_CAPACITY. */
MGF_API mgf_status mgf_world_add_compound_bodies(mgf_world* w, const mgf_component* comps, const float* comp_mass,
                                                 const int64_t* offsets /* n + 1 */, int64_t n, const float* restitution,
                                                 const float* friction, const mgf_vec3* world_force, uint64_t* first_id);
MGF_API int64_t mgf_world_len(const mgf_world* w);
/* One tick (world.rs:227-294): complete_motion, integrate, broadphase, narrowphase,
 * ContactConstraint::new for every contact, Solver::solve(iters). */
MGF_API mgf_status mgf_world_step(mgf_world* w, float dt, int32_t iters, mgf_step_stats* stats);
/* n ticks back to back (World::step in a host loop); stats (optional) receives one record per tick.  Same results as n
 * calls of mgf_world_step; with a dataflow solver tick k + 1 is enqueued before tick k's counts are read back, and a
 * device-side guard makes it a no-op when tick k has to be re-run with larger lists (option "pipeline" [1]). */
MGF_API mgf_status mgf_world_step_many(mgf_world* w, float dt, int32_t iters, int64_t n, mgf_step_stats* stats);
/* Same tick split at the solver boundary (for parity tests of the constraint list). */
MGF_API mgf_status mgf_world_build_constraints(mgf_world* w, float dt, mgf_step_stats* stats);
MGF_API mgf_status mgf_world_solve(mgf_world* w, int32_t iters, mgf_step_stats* stats);   /* Solver::solve solver.rs:72 */
/* RigidBodyVec::{complete_motion, integrate} alone (physics.rs:262, 222). */
MGF_API mgf_status mgf_world_complete_motion(mgf_world* w);
MGF_API mgf_status mgf_world_integrate(mgf_world* w, float dt);
/* ConstrainedSet::get / set (physics.rs:272-315). */
MGF_API mgf_status mgf_world_get(mgf_world* w, const mgf_body_ref* r, mgf_velocity* vel, mgf_rigid_body_info* info);
MGF_API mgf_status mgf_world_set(mgf_world* w, const mgf_body_ref* r, const mgf_velocity* vel);
/* Bulk state access; any pointer may be NULL.  delta = collider[i].1 (Moving displacement).  What is asked for is packed on the device in
 * the caller's body order and crosses PCIe once, through pinned memory (all five arrays of 262 144 bodies: 0.9 ms either way). */
MGF_API mgf_status mgf_world_read_state(mgf_world* w, mgf_vec3* x, mgf_quat* q, mgf_vec3* v, mgf_vec3* omega,
                                        mgf_vec3* delta, int64_t cap);
MGF_API mgf_status mgf_world_write_state(mgf_world* w, const mgf_vec3* x, const mgf_quat* q, const mgf_vec3* v,
                                         const mgf_vec3* omega, const mgf_vec3* delta, int64_t n);
MGF_API mgf_status mgf_world_read_colliders(mgf_world* w, mgf_moving_component* out, int64_t cap); /* colliders() :256 */
/* ---- queries against the world between ticks (NOT in the reference: its World is the demo's, so the definition is this
 * build's; DESIGN.md "world queries").  A query sees each owned body's collider at its current pose as mgf_world_read_colliders
 * returns it (the Moving displacement is not swept) - for a body of several components each of its parts in world coordinates -
 * the terrain's faces and each obstacle as Intersects<Compound> (compound.rs:309-332) at its pose.  Ghost bodies are never
 * reported; the tick's state is not touched (a step after a query is bit-identical to one without it). ----
 * Ray cast: per particle (a Ray has dt = INFINITY, a Segment dt = 1) the closest hit of Intersects<shape> (collision.rs:169-373;
 * compound.rs:150 for a component): the smallest t, ties to the target first in the order bodies (ascending caller index, a body's
 * parts in order), terrain faces (ascending index), obstacles (in the order added).  inter is bit-identical to that single test.
 * kind: MGF_HIT_NONE (-1, the other fields zero), MGF_HIT_BODY (index = the caller's body index), MGF_HIT_TERRAIN (index = face),
 * MGF_HIT_OBSTACLE (index = obstacle); part = the component within a body of several components or within an obstacle (else 0).
 * A particle with d = 0 hits nothing (the single tests divide by |d|^2 there: every sphere would answer at t = 0).
 * More generally a particle is cast only if the largest |component| of d lies in [MGF_RAY_DMIN, MGF_RAY_DMAX]; outside that band - and
 * for a d with a NaN - it hits nothing.  Outside it the single tests stop being local: |d|^2 underflows or the discriminants overflow,
 * and a sphere or a capsule nowhere near the line answers at t = 0, inf or NaN (EXPERIMENTS.md, "the direction band of a ray").
 * A hit whose t is not finite is not a candidate (the sweeps' rule, below): whatever target offers it, it is passed over.
 * The single tests are not local for an origin far away either, and their answers stand as the definition's: ray_sphere decides by the sign
 * of b^2 - a c, which cancels, so a sphere of radius r whose centre is m from the origin answers when the line passes its centre within
 * sqrt(r^2 + 1e-6 m^2) - from 1e5 away a body 50 off the line can be the hit.  The walk is laid over the grid's box grown by that tube,
 * cells beside the grid included, and looks that far around the line at each; where the tube is more than two cells a particle whose path
 * meets the grown box is put to every body.  The bound is the spheres' and the capsules' end caps'; the cylinder test of
 * a capsule divides the same noise by sin^2 of the angle between particle and axis, so a particle that runs nearly along a far capsule's
 * axis may be answered from further off than the walk looks: a stated limit (the batch's bounding-sphere reject allows 1e-2 m). */
#define MGF_RAY_DMIN 1e-20f
#define MGF_RAY_DMAX 1e12f
#define MGF_HIT_NONE (-1)
#define MGF_HIT_BODY 0
#define MGF_HIT_TERRAIN 1
#define MGF_HIT_OBSTACLE 2
#define MGF_QUERY_BODIES 1
#define MGF_QUERY_TERRAIN 2
#define MGF_QUERY_OBSTACLES 4
#define MGF_QUERY_ALL 7
typedef struct mgf_ray_hit { int32_t kind; int32_t index; int32_t part; mgf_intersection inter; } mgf_ray_hit;
/* ignore_body: NULL, or n caller body indices (-1: none) that particle i skips; kinds_mask: MGF_QUERY_* bits (0 is refused). */
MGF_API mgf_status mgf_world_raycast_many(mgf_world* w, const mgf_particle* parts, int64_t n, const int32_t* ignore_body,
                                          int32_t kinds_mask, mgf_ray_hit* out);
/* Sweep: per cast (a sphere, tag 0, or a capsule, tag 1, in world coordinates, swept by delta) the earliest contact of the target's
 * continuous test, the target the receiver and the cast Moving::sweep(shape, delta):
 *   body       every component of an owned body's collider at its current pose (as mgf_world_read_colliders and, for a body of several
 *              components, its world parts give it; the collider's own delta is not applied): Contacts<Moving<Sphere | Capsule>> of that
 *              sphere or capsule (collision.rs:1089-1356; Sphere vs Moving<Capsule> through commute_contacts!, :1143);
 *   terrain    each face, the mesh's position added: Contacts<Moving<_>> for Poly (collision.rs:610-1000), up to two contacts for a
 *              capsule, in the order it emits them;
 *   obstacle   Compound::contacts(&Moving::sweep(shape, delta)) at the obstacle's pose (compound.rs:334-351); part = the component.
 * Among all contacts of the selected kinds the one with the least (t, kind, index, part, order emitted within that one target) is
 * reported; every part of ignore_body[i] is skipped; ghosts are never reported.  contact is bit-identical to the single test's: a on
 * the target, b on the cast, both at time t, n as the target's test emits it.  No contact: kind MGF_HIT_NONE, every other field zero.
 *   delta = 0 is a valid cast: the single tests report a cast that starts overlapping a target at t = 0 (except sphere on sphere with
 *   equal centres, which reports nothing, collision.rs:1097-1100).
 *   The face test of a capsule is not local, and its answers stand as the definition's: its axis test (collision.rs:698-719) measures
 *   along the unit axis and steps along the whole one, so it answers at t = 0 for a capsule up to max(1, |d|) from a face; with
 *   delta = 0 its fallback (:901-1060) casts rays of direction 0, which can answer at t = 0 at any face.
 *   A contact whose t is not finite is not a candidate: a capsule whose length overflows f32 (d finite, |d| = inf) makes the face test
 *   emit t = NaN beside finite contacts (collision.rs:693-1086).
 * ignore_body: NULL, or n caller body indices (-1: none); kinds_mask: MGF_QUERY_* bits (0 is refused); a tag other than 0 or 1 is
 * refused (MGF_ERR_INVALID). */
typedef struct mgf_sweep_hit { int32_t kind; int32_t index; int32_t part; mgf_contact contact; } mgf_sweep_hit;   /* 52 bytes */
MGF_API mgf_status mgf_world_sweep_many(mgf_world* w, const mgf_moving_component* casts, int64_t n, const int32_t* ignore_body,
                                        int32_t kinds_mask, mgf_sweep_hit* out);
/* Box overlap: per mgf_aabb every owned body whose tight bound BoundedBy<AABB> (bounds.rs:170-190; for a body of several components
 * the union of its parts' bounds) passes Overlaps<AABB> (collision.rs:22), in ascending caller index: out_bodies[out_offsets[q] ..
 * out_offsets[q+1]); a box with a NaN or a negative half extent answers as that test does.  As mgf_bvh_query_many: out_offsets and
 * *total are always filled; MGF_ERR_CAPACITY if *total > cap. */
MGF_API mgf_status mgf_world_overlap_aabb_many(mgf_world* w, const mgf_aabb* boxes, int64_t n, uint64_t* out_offsets /* n+1 */,
                                               uint32_t* out_bodies, int64_t cap, int64_t* total);
/* The Solver's constraint list of the last tick, in insertion order. */
MGF_API mgf_status mgf_world_read_constraints(mgf_world* w, mgf_constraint* out, int64_t cap, int64_t* count);
/* Solver::add_constraint in bulk + solve on the resident RigidBodyVec (solver.rs:66-78):
 * replaces the tick's constraint list with `cons` (insertion order = array order). */
MGF_API mgf_status mgf_world_set_constraints(mgf_world* w, const mgf_constraint* cons, int64_t n);
/* ---- the library-level pieces World::step is assembled from, on their own (a caller that does its own collision
 * detection builds manifolds, constraints and a Solver exactly as mgf_demo/world.rs:243-251,279-291 does) ----
 * ContactConstraint::new(pool, obj_a, obj_b, manifold, dt) (solver.rs:101-191) for n caller-built manifolds on the world's
 * resident RigidBodyVec (mix of restitution / friction, bias, normal and tangent masses from ConstrainedSet::get of both
 * bodies).  refs_a[i] must be Dynamic (MGF_ERR_STATIC_REF otherwise: every call site of the reference passes one);
 * refs_b[i] Dynamic or Static{center, friction}.  The manifold's normal and tangent vectors are used as given.  A manifold
 * of m contacts yields m consecutive single-contact records that share its normal and tangents - equivalent under
 * ContactConstraint::solve (solver.rs:219-248: the contacts one after the other on the same velocities).  *count = records
 * written (MGF_ERR_CAPACITY if cap is smaller; *count still reports the number required). */
MGF_API mgf_status mgf_constraints_new(mgf_world* w, const mgf_body_ref* refs_a, const mgf_body_ref* refs_b, const mgf_manifold* manifolds,
                                       int64_t n, float dt, mgf_constraint* out, int64_t cap, int64_t* count);
/* Solver<ContactConstraint> (solver.rs:53-79): new / add_constraint (bulk form too) / solve(&mut rbv, iters) / len.  The
 * handle owns its insertion-ordered list; solve runs it on the world's RigidBodyVec in the exact sequential order, with
 * the tick's executors (the world's own tick list is replaced, as by mgf_world_set_constraints), and the constraints keep
 * their state (normal_impulse) between solve calls as the reference's do.  mgf_solver_clear is `Solver::new()` again
 * (world.rs:228 rebuilds the solver every tick). */
MGF_API mgf_status mgf_solver_new(mgf_solver** out);                                              /* Solver::new            solver.rs:59 */
MGF_API void mgf_solver_free(mgf_solver* s);
MGF_API mgf_status mgf_solver_add_constraint(mgf_solver* s, const mgf_constraint* c);             /* Solver::add_constraint solver.rs:66 */
MGF_API mgf_status mgf_solver_add_constraints(mgf_solver* s, const mgf_constraint* cons, int64_t n);
MGF_API int64_t mgf_solver_len(const mgf_solver* s);
MGF_API mgf_status mgf_solver_clear(mgf_solver* s);
MGF_API mgf_status mgf_solver_read_constraints(const mgf_solver* s, mgf_constraint* out, int64_t cap, int64_t* count);
MGF_API mgf_status mgf_solver_solve(mgf_solver* s, mgf_world* w, int32_t iters, mgf_step_stats* stats); /* Solver::solve solver.rs:72 */
/* RigidBodyVec: Clone (physics.rs:140), with the rest of the world it lives in (terrain copy, parameters, options): an
 * independent world on the same context that steps bit-identically.  Ghosts and the tick's lists are not copied. */
MGF_API mgf_status mgf_world_clone(mgf_world* src, mgf_world** out);
/* ContactPruner::new + push(contact) for every LocalContact of a group, in order, then Manifold::from(pruner)
 * (manifold.rs:42-148) for n groups at once: group i = contacts[offsets[i] .. offsets[i+1]).  params = NULL uses
 * DefaultPruningParams / COLLISION_EPSILON.  The reference's pruner is unbounded; a group that keeps more than
 * MGF_MANIFOLD_CAP contacts returns MGF_ERR_CAPACITY (its n_contacts still reports the count). */
MGF_API mgf_status mgf_manifolds_from_contacts(mgf_ctx* ctx, const mgf_params* params, int64_t n, const uint64_t* offsets,
                                               const mgf_local_contact* contacts, mgf_manifold* out);
/* ---- scene I/O: the serde_json shape of the reference's persistent types (bvh.rs:29-47, pool.rs:25-41, mesh.rs:31-37,
 * geom.rs:256-260; cgmath vectors as {"x","y","z"}).  *_to_json writes a NUL-terminated string; *len is its length
 * (MGF_ERR_CAPACITY if cap < *len + 1).  *_from_json rebuilds the identical tree - entry for entry, free list included -
 * so later inserts reuse the same slots as in the process that wrote the file. */
MGF_API mgf_status mgf_bvh_to_json(const mgf_bvh* b, char* buf, int64_t cap, int64_t* len);
MGF_API mgf_status mgf_bvh_from_json(mgf_ctx* ctx, const char* json, int64_t len, mgf_bvh** out);
MGF_API mgf_status mgf_mesh_to_json(const mgf_mesh* m, char* buf, int64_t cap, int64_t* len);
MGF_API mgf_status mgf_mesh_from_json(mgf_ctx* ctx, const char* json, int64_t len, mgf_mesh** out);
/* The geometry structs of geom.rs:31-357 in serde_json's shape: s->kind selects the struct - MGF_SPHERE {"c","r"},
 * MGF_CAPSULE {"a","d","r"}, MGF_TRIANGLE {"a","b","c"}, MGF_PLANE {"n","d"}, MGF_RECTANGLE {"c","u":[V,V],"e":[f,f]} (v = c, u0,
 * u1, e0, e1), MGF_RAY {"p","d"}, MGF_SEGMENT {"a","b"}, MGF_AABB {"c","r"}; V = {"x","y","z"}.  moving != NULL writes / reads
 * Moving<T>(T, Vector3<f32>), a tuple struct, i.e. [T, V] (geom.rs:356-357; `Component` itself derives no Serialize).
 * Reading follows serde's struct rules: fields in any order, unknown fields ignored, missing or duplicate field = error. */
MGF_API mgf_status mgf_geom_to_json(const mgf_shape* s, const mgf_vec3* moving, char* buf, int64_t cap, int64_t* len);
MGF_API mgf_status mgf_geom_from_json(int32_t kind, const char* json, int64_t len, mgf_shape* out, mgf_vec3* moving);
/* ---- Compound (compound.rs:230-352): a static aggregate of spheres and capsules with a pose and an internal BVH ----
 * mgf_compound_new = Compound::new (components inserted into the BVH in order); set_pose writes the pub fields
 * disp / rot (rot is assumed normalised, as in the reference); contacts_many = Contacts<RHS> for Compound with
 * RHS = Moving<Sphere> / Moving<Capsule> for n moving components at once (per rhs: the contacts in the order the
 * reference's callback receives them, CSR offsets); intersections = Intersects<Compound> for n particles;
 * bounds = BoundedBy<AABB> (MGF_ERR_EMPTY for an empty compound, bvh.rs:265). */
MGF_API mgf_status mgf_compound_new(mgf_ctx* ctx, const mgf_component* comps, int64_t n, mgf_compound** out);
MGF_API void mgf_compound_free(mgf_compound* c);
MGF_API mgf_status mgf_compound_set_pose(mgf_compound* c, mgf_vec3 disp, mgf_quat rot);
MGF_API mgf_status mgf_compound_bounds(const mgf_compound* c, mgf_aabb* out);
MGF_API mgf_status mgf_compound_contacts_many(mgf_compound* c, const mgf_moving_component* rhs, int64_t n, uint64_t* out_offsets,
                                              mgf_contact* out, int64_t cap, int64_t* total);
MGF_API mgf_status mgf_compound_intersections(mgf_compound* c, const mgf_particle* parts, int64_t n, mgf_intersection* out,
                                              int32_t* hit);
/* ---- spatial tiling across the GPUs of a node (one process per GPU) -----------
 * A tick on a tile is begin_tick -> [select_boundary, export_bodies -> neighbour -> import_ghosts]
 * -> collide -> iters x { solve(1) -> [export_velocities -> neighbour -> import_ghost_velocities] }.
 * Ghost bodies are local copies of a neighbour tile's boundary bodies; they collide with owned
 * bodies only (their terrain contacts and ghost-ghost pairs belong to their owner).  All buffers
 * below are DEVICE pointers owned by the caller (e.g. the exchange buffers handed to RCCL).
 * Ghost record: MGF_GHOST_FLOATS = 72 floats  x3 q4 v3 w3 delta3 | tag p3 d3 r | inv_mass I9 restitution friction | n_parts, 3 pad |
 * 4 x (p3 r d3 kind) world parts of a body of several components (zeros otherwise);
 * velocity record: 8 floats v3 w3 0 0. */
MGF_API mgf_status mgf_world_begin_tick(mgf_world* w, float dt);     /* complete_motion + integrate (world.rs:230-231) */
MGF_API mgf_status mgf_world_collide(mgf_world* w, float dt, mgf_step_stats* stats); /* world.rs:233-291 */
/* Owned bodies whose fat AABB reaches below x_left / above x_right, ascending ids. */
MGF_API mgf_status mgf_world_select_boundary(mgf_world* w, float x_left, float x_right, uint32_t* ids_left,
                                             uint32_t* ids_right, int64_t cap, int64_t* n_left, int64_t* n_right);
MGF_API mgf_status mgf_world_export_bodies(mgf_world* w, const uint32_t* ids, int64_t n, float* dst);
MGF_API mgf_status mgf_world_import_ghosts(mgf_world* w, const float* src, int64_t n_ghost);
MGF_API mgf_status mgf_world_export_velocities(mgf_world* w, const uint32_t* ids, int64_t n, float* dst);
MGF_API mgf_status mgf_world_import_ghost_velocities(mgf_world* w, const float* src, int64_t n_ghost);
MGF_API int64_t mgf_world_ghost_len(const mgf_world* w);
/* ---- migration: an owned body whose centre leaves its tile's slab [x_lo, x_hi) changes owner -------
 * mgf_world_select_tile = mgf_world_select_boundary + the migrants of this tick: counts[0..1] boundary bodies
 * (left, right), counts[2..3] bodies with centre.x < x_lo / >= x_hi; ids_migrants receives the left-goers then the
 * right-goers (each ascending), at most cap in total.  A tick without migrants costs one extra counting kernel and
 * no extra host wait.  The tiles driver (mgf_amd/tiles.py) moves the selected bodies at the END of the tick:
 * export_migrants (MGF_MIGRANT_FLOATS floats per body: the body's row of every device array, fat AABB and tag
 * included) -> neighbour -> remove_bodies on the old owner, import_migrants (append) on the new one.  Ids of the
 * remaining bodies shift down on removal; mgf_world_set_tags / read_tags give bodies an identity that survives. */
#define MGF_GHOST_FLOATS 72
#define MGF_MIGRANT_FLOATS 148
MGF_API mgf_status mgf_world_select_tile(mgf_world* w, float x_left, float x_right, float x_lo, float x_hi,
                                         uint32_t* ids_left, uint32_t* ids_right, uint32_t* ids_migrants, int64_t cap,
                                         int64_t* counts /* [4] */);
MGF_API mgf_status mgf_world_export_migrants(mgf_world* w, const uint32_t* ids, int64_t n, float* dst);
MGF_API mgf_status mgf_world_remove_bodies(mgf_world* w, const uint32_t* ids, int64_t n);  /* distinct ids, any order */
MGF_API mgf_status mgf_world_import_migrants(mgf_world* w, const float* src, int64_t n);
MGF_API mgf_status mgf_world_set_tags(mgf_world* w, const uint32_t* tags /* host, one per owned body */, int64_t n);
MGF_API mgf_status mgf_world_read_tags(mgf_world* w, uint32_t* tags /* host */, int64_t cap);
/* Stream-ordered variant of the loop above, for a driver that issues its RCCL transfers on the context's
 * stream (mgf_ctx_set_stream): with option "stream_ordered" = 1 begin_tick / select_boundary's scatter /
 * export_* / import_* only enqueue; mgf_world_solve_enqueue is Solver::solve without the read-back, and
 * mgf_world_finish synchronises once and reports the outcome (status, timings) of everything enqueued. */
MGF_API mgf_status mgf_world_solve_enqueue(mgf_world* w, int32_t iters);
MGF_API mgf_status mgf_world_finish(mgf_world* w, mgf_step_stats* stats);
/* ---- the whole tile protocol under the C-ABI (what a Rust host calls once per tick; mgf_amd/tiles.py is the same protocol in
 * Python, kept as the transport-agnostic reference driver of the CPU tests).  A process owns n_local consecutive x-slab
 * tiles [first_tile, first_tile + n_local) of n_tiles_total, each a mgf_world on the same context with its slab
 * [x_lo, x_hi).  mgf_tiles_step runs one tick of all of them: begin_tick + boundary / migrant selection of every tile with ONE
 * host wait, ghost bodies to the neighbours, collide of every tile enqueued before the first read-back is waited for,
 * iters / refresh_every x { Solver::solve(refresh_every); ghost velocities from their owners }, finish, hand-over of bodies
 * whose centre left their slab.  Between tiles of one process the exchange is a device copy; between processes (one per GPU)
 * it is RCCL point-to-point (ncclSend / ncclRecv in one group per exchange step, on the context's stream, over xGMI):
 * rank 0 calls mgf_rccl_unique_id, the host program hands the 128 bytes to the other ranks, every rank calls
 * mgf_tiles_connect(rank, n_ranks) - rank r's tile range follows rank r - 1's - and mgf_tiles_preflight sums a 1 from every
 * rank over the communicator (0 = not connected).  librccl is loaded at run time, on the first of these calls.
 * stats (optional) receives one record per local tile.  Results are bit-identical to mgf_amd/tiles.py and to the oracle's
 * tile mode, and independent of how the tiles are spread over processes.
 * (Between its own tiles and ranks mgf_tiles_step moves narrower records than the calls above hand to a caller: a world without bodies
 * of several components sends the first 40 floats of a ghost record - the receiver learns the width from the kinds its neighbour announces
 * with its counts - and velocity records are 6 floats, v3 w3.) */
MGF_API mgf_status mgf_tiles_create(mgf_ctx* ctx, int32_t n_local, mgf_world* const* worlds, const float* x_lo, const float* x_hi,
                                    int32_t first_tile, int32_t n_tiles_total, float halo, int32_t refresh_every, int32_t migrate,
                                    mgf_tiles** out);
MGF_API void mgf_tiles_free(mgf_tiles* t);
MGF_API mgf_status mgf_rccl_unique_id(void* id128);
/* Which library provides ncclSend / ncclRecv: librccl.so by default, whatever the environment says.  After
 * mgf_rccl_allow_override(1) - called by the host program before any other mgf_rccl_* / mgf_tiles_connect call - the environment
 * variable MGF_RCCL_LIB may name another one (a site's own RCCL build; the test-suite's stand-in transport). */
MGF_API mgf_status mgf_rccl_allow_override(int32_t allow);
MGF_API mgf_status mgf_tiles_connect(mgf_tiles* t, const void* id128, int32_t rank, int32_t n_ranks);
MGF_API mgf_status mgf_tiles_preflight(mgf_tiles* t, int32_t* n_ranks_seen);
MGF_API mgf_status mgf_tiles_step(mgf_tiles* t, float dt, int32_t iters, mgf_step_stats* stats /* n_local, or NULL */);
/* Options of a tile set.  "exchange_timing" [0]: HIP events around every neighbour exchange feed the counter "exchange_ns" (an event is
 * a barrier packet in the stream: off unless asked for).  "test_fail_tick" = the mgf_tiles_step call (0-based) in which this rank fails on purpose in its collide
 * phase: the protocol's status agreement is then observable (no rank hangs, every rank reports the tick as lost); -1 = never.
 * "retry_lost_ticks" [1]: a tick in which a persistent solver launch gave up on any rank (a device shared with another process) is repeated
 * on every rank - the tiles' owned bodies put back to where the tick found them, the launch-per-frontier executor for the next solves;
 * Solver::solve has no failure mode, solver.rs:72-78 - instead of being reported as lost (counter "ticks_retried"). */
MGF_API mgf_status mgf_tiles_set_option(mgf_tiles* t, const char* key, int64_t value);
MGF_API int64_t mgf_tiles_migrated(const mgf_tiles* t, int32_t tile, int32_t direction_in); /* bodies handed over so far */
/* What the neighbour exchanges of a tile set have cost since its creation (no reference counterpart: world.rs has one World): key =
   "exchange_bytes_out" / "exchange_bytes_in" (rows that crossed a face between RANKS), "exchange_bytes_local" (rows copied between this
   rank's own tiles), "exchange_calls", "exchange_ns" (stream time between the events around the exchanges, the wait for the neighbouring
   rank included; counted while mgf_tiles_set_option "exchange_timing" is 1) and, by kind of exchange, "exchange_{calls|mean_ns|p50_ns|p99_ns|max_ns}_{bodies|
   velocities|handover}" (the calls' own durations: which step of the protocol costs what on the links), "host_waits", "ticks", "ticks_retried"; -1 for an unknown key. */
MGF_API int64_t mgf_tiles_counter(const mgf_tiles* t, const char* key);
/* Options (development and test knobs; defaults in brackets): "time_solver_kernels" [0] HIP events around the
 * solver kernels; "solver_mode" [6] 1 = persistent dataflow launch, 0 = one launch per dependency frontier,
 * 4 = dataflow with out-of-order slots, 5 = block-local dataflow (velocities and counters of a spatial block in LDS),
 * 6 = block-local dataflow with message channels between the blocks (every body a block touches in LDS);
 * (modes 1, 4, 5, 6 are persistent launches whose workgroups wait for one another: they need the device's compute units to
 * themselves - one process per GPU, one context's stream at a time.  Where two processes' launches overlap on one device each
 * may hold part of the compute units; a launch then gives up after about half a second.  Solver::solve cannot fail (solver.rs:72-78), so
 * neither does the call: mgf_world_step / _step_many / _solve put the velocities (and accumulated impulses) back as the launch found
 * them and solve the list again with the launch-per-frontier executor - bit-identical - counted in "solver_abort_fallbacks"; a tile set
 * repeats the tick on every rank ("retry_lost_ticks").  MGF_ERR_HIP "dataflow solver gave up waiting" can still surface only where
 * nothing can be solved again from inside the call: "stream_ordered" = 1 (no wait inside the call), or a tile set with
 * "retry_lost_ticks" = 0 - the state is then that of a tick whose solve did not happen.  Processes that know they share a device say
 * so with "flow_max_blocks");
 * "constraint_order" [0] 1 = the reference's own insertion order, replayed on the host (world.rs:233-291);
 * "pair_brick" [1] (grid broadphase with an 8x8x8-cell box staged in LDS; 0 = every look-up from global memory);
 * "grid_min_frac_pct" [50] (axes of the scene shorter than this percentage of the longest one are widened to it before
 * the Morton cells are laid over it: cells stay near-cubic in an x-slab tile);
 * "flow6_fcap", "flow6_const_lds", "flow6_poll_waves", "flow6_test_cap" (mode 6: foreign-body slots, constants in LDS,
 * polling waves, a test limit that forces the stand-by kernel); "two_pass_candidates" [0]; "broadphase_tree" [0]; "terrain_tree" [0]; "no_fused_narrowphase" [0] (a world of spheres only runs the sphere-sphere test inside the grid broadphase and lists contacts only; 1 = list every accepted partner); "stream_ordered" [0]; "phase_timing" [0] (HIP events at the tick's phase boundaries: mgf_step_stats::ms_*), "time_solver_kernels" [0] (events around the solver launches: ms_solver_kernels); "pipeline" [1] (mgf_world_step_many enqueues the next tick before it waits for this one); "cell_fill" [16] (bodies per Morton cell, in eighths, beyond which the broadphase grid gets another level); "no_fused_terrain_rows" [0], "no_fused_scene_bounds" [0] (mgf_world_step and mgf_world_begin_tick list the terrain faces of a body and gather the scene bounds inside the integration kernel; 1 = always the separate kernels); "list_capacity";
 * "fused_contacts" [1] (a world of spheres over a small mesh: rows -> constraint records without candidate lists; 0 = the candidate-list kernels);
 * "contacts_split" [1] (the launch that writes the constraint records from the rows in two: the numbering - ids, (a, b), the bodies' rows of
 * `b` occurrences - ahead of the block-local solver's table kernels, the partner contacts' 128-byte records beside them, as foreign blocks of the
 * links launch; where no tables are built inside the collide phase, a launch of their own behind the numbering.  2 = the record blocks first in that
 * launch, 3 = a launch on the context's second stream, 4 = always a launch of their own: experiments; 0 = one launch, k_contacts_rows);
 * "scan_fused" [1] (a world of spheres with contacts_split on: the constraint numbering - the prefix sum of the bodies' constraint counts and the
 * tick's list sizes - inside the numbering launch itself; 0 = a prefix-sum launch of its own ahead of it.  The results are the same bit for bit);
 * "tables_fused" [1] (with scan_fused, the block-local solver and a store kept in cell order - resort_every - whose solver blocks hold at most
 * 1 024 bodies: the numbering launch takes a ticket per solver block and also writes that block's part of the solver's tables - the bodies'
 * look-up words, the foreign bodies, every own constraint's row; 0 = a launch of its own behind it, which every other world keeps.  The results
 * are the same bit for bit);
 * "front_rows" [1] (r06: a world of single-component bodies that are not all spheres - capsules, mixed - or of bodies of up to two components:
 * the pair search runs the pair test on the partners it accepts, the bodies near the mesh get their faces and the body-triangle test in
 * launches of their own, the constraint records are written from the rows; 0 = candidate lists and one narrowphase launch per shape-pair
 * type); "front_rows_check" [0] (tests: the faces the cheap conservative reject ahead of the body-triangle tests drops are tested all the
 * same - a contact among them is reported as an internal error); "side_stream" [1] (the terrain kernels of that front end run on a
 * second stream of the context beside the pair search; 0 = everything on the context's stream; 3 = the fork and the join without the second
 * stream: what the two events cost by themselves);
 * "wide_list" [1] (r06: the few bodies whose fat box is far larger than the rest's - a body that left the scene and falls at 200 m/s - are kept
 * out of the scene bounds and of the reach of every query of the cell grid, and paired by a launch of their own; the accepted set is the
 * reference's either way (bvh.rs:283-310); engaged by the host from the tick after such a body shows;
 * 0 = never);
 * "cells_in_integrate" [1] (the fused tick's k_integrate works out the bodies' Morton cells over the previous tick's scene bounds);
 * "flow_max_blocks" [0] (the persistent solver launches of this world take at most this many workgroups - one per CU; 0 = all CUs.  Processes that
 * share a device each take a part, so that their launches are resident together); "flow_spin_limit" [0] (tests: 1 = every other workgroup of a
 * persistent launch returns at once and the launch gives up - the world then restores its pre-launch velocities and solves the list with the
 * launch-per-frontier executor, counter "solver_abort_fallbacks");
 * "flow6_foreign_lds" [1], "flow6_nimp_lds" [1], "flow6_rec_lds" [1] (mode 6: the foreign bodies' constants, the accumulated normal impulses and
 * the solver half of the constraint records in LDS where there is room; 0 = never), "flow6_slot_margin" [0] (what the LDS split lets a block's
 * slots grow over the last tick's largest block), "flow6_quad" [1] and "flow6_quad_max" [-1] (four lanes per node while the ready queue is short;
 * -1 = chosen by the launch), "flow6_spec" [0] and "flow6_spec_wl" [-1] (positions the polling waves read on spec; chosen by the launch);
 * "resort_every" [-1] (ticks between two re-sorts of the body store into compact spatial blocks in the fused tick; 0 = the caller's order, -1 =
 * automatic); "readback_kernel" [1] (the tick's read-back is written to pinned memory by a kernel and polled; 0 = a copy command and an event);
 * "flow_trace" [0] (development: per-node timestamps of a dataflow launch); "flow5_block" [0] (tests: the minimum bodies per block of the
 * block-local solvers), "flow5_test_cap" [0] (tests: a limit on a block's constraints that forces mode 5's stand-by kernel); "body_kinds" (OR-in, bit0 sphere, bit1 capsule): the
 * kinds this world's ghosts may have - a tile whose own bodies are all of one kind must be told when a neighbour's are
 * not, because the narrowphase dispatch is chosen on the host (the tiles driver exchanges the masks with the counts). */
MGF_API mgf_status mgf_world_set_option(mgf_world* w, const char* key, int64_t value);
/* Diagnostics: how often a slow path was taken.  name in {"row_overflows", "capacity_retries", "flow5_fallbacks",
 * "grid_too_wide", "flow5_blocks", "flow5_class0|1|2", "terrain_grid", "terrain_row_capacity", "rev_row_capacity", "body_kinds",
 * "flow6_fallbacks", "flow6_fail_reason", "flow6_max_slots", "flow6_max_foreign", "pair_brick_slow_queries", "pair_brick_off_ticks",
 * "max_fat_half_extent_x_milli", "scene_rmax_milli_x|y|z", "scene_ext_milli_x|y|z", "grid_levels", "front_rows", "front_near", "front_faces",
 * "front_slots" (the list-free front end of the last tick: bodies near the mesh, faces accepted, faces that passed the cheap reject),
 * "wide_bodies" (listed in the last tick), "wide_ticks", "wide_overflows" (ticks run again because more bodies were wide than the list holds),
 * "flow6_skipped" (plans that declined the block-local solver because the last launch that did not fit says it still would not), "solver_abort_fallbacks" (Solver::solve calls whose persistent launch gave up and that were solved again from
 * the pre-launch state: Solver::solve has no failure mode, solver.rs:72-78), "device_ptrs_out" (1 while mgf_world_device_ptr's pointers pin
 * the store to the caller's order), "query_large_bodies" / "query_cells" (the last world query's large-body list and grid),
 * "query_build_ns" / "query_run_ns" (HIP-event times of its grid build and of its query pass), "pair_brick_ticks", "front_rows_ticks",
 * "fused_contacts_ticks", "early_cells_ticks" (ticks whose collide phase settled on k_pair_brick, on the list-free front end, on
 * k_contacts_spheres without candidate lists, on cells worked out inside k_integrate), "two_pass_ticks", "tree_ticks", "big_parts_ticks"
 * (ticks whose candidate lists were counted and filled in two passes, whose pair search walked the tree instead of the cell grid, whose
 * narrowphase ran the kernels for bodies of more than four components), "contacts_split_fused" / "contacts_split_standalone" (ticks whose partner
 * records were written beside the links launch / by a launch of their own; both 0: option contacts_split = 0 or another front end),
 * "scan_fused_numbering_ticks" (ticks whose constraints were numbered inside the numbering launch: option scan_fused; a tick that was run again
 * counts in none of these), "tables_fused_ticks" (ticks whose solver tables were built inside that launch: option tables_fused; ticks run again
 * count in neither), "scan_fused_run" / "scan_fused_look" (bodies per ticketed run of that launch, runs read per sweep of its look-back),
 * "contacts_records_pending" (tests: 1 only inside a collide phase being enqueued), "max_parts" (the most components any body has)}. */
MGF_API mgf_status mgf_world_counter(const mgf_world* w, const char* name, int64_t* out);
/* Raw device pointers of resident state for zero-copy exchange (multi-GPU halo): name in
 * {"x","q","solver_rec","delta"} (the pub fields `x`, `q` of RigidBodyVec physics.rs:142-154 and what ConstrainedSet::get returns,
 * :273-288), rows indexed by the caller's body index.  Valid until the next add_bodies / remove_bodies.  While pointers are out the
 * world keeps its store in the caller's order (the fused tick does not re-sort it into cell order: slower ticks, same results);
 * mgf_world_release_device_ptrs gives them back - after it the pointers must not be used. */
MGF_API mgf_status mgf_world_device_ptr(mgf_world* w, const char* name, void** ptr, int64_t* bytes);
MGF_API mgf_status mgf_world_release_device_ptrs(mgf_world* w);

/* ---- many small worlds (NOT in the reference: world.rs has one World; DESIGN.md "many small worlds") ----------------------------
 * A batch of n_worlds independent worlds, resident in HBM, stepped together: ONE kernel launch per tick whatever n_worlds is, one
 * workgroup per world, no host wait between the ticks of a call.  Per world the definition is exactly World::step
 * (mgf_demo/world.rs:227-294) in the canonical constraint order, as mgf_world_step computes it: complete_motion + integrate
 * (physics.rs:222-269), the fat-box refit rule (world.rs:235-238), Mesh::contacts in mesh-BVH DFS order with every contact a constraint of
 * its own (world.rs:243-251), the partners j < i ascending through ContactPruner / Manifold / ContactConstraint::new
 * (manifold.rs:72-148, solver.rs:101-191), Solver::solve (solver.rs:72-78).  Worlds never interact; what world k computes does not
 * depend on what else is in the batch or on where in it the world sits.  No workgroup waits for another: a batch may hold more
 * worlds than the device holds workgroups, and it is safe on a device shared with another process.
 * LIMITS: bodies of one to four components (spheres and capsules; mgf_batch_add_compound_bodies below - the lone world takes 32, a body
 * of 5..32 is refused here); on a batch that holds a body of more than one component the calls that read the shapes of bodies -
 * mgf_batch_raycast_many(_dev), _sweep_many(_dev), _overlap_aabb_many, _overlap_first_dev, _cast_sensors(_dev), _cast_cameras(_dev),
 * _read_zones(_dev), _cast_feelers(_dev) - return MGF_ERR_INVALID ("... several components ..."), enqueue nothing and change nothing: they do not see
 * parts yet (the set_* calls of the rigs stay as they are); at most MGF_BATCH_MAX_BODIES bodies per world, counted in bodies, not parts (a call that would exceed it
 * is refused with MGF_ERR_INVALID and adds nothing); the static geometry of a world is one terrain mesh, or none: an entry of the
 * batch's terrain table (meshes are copied in; any number of worlds may share an entry) at a position of the world's own, and beside it
 * up to MGF_BATCH_MAX_WORLD_OBSTACLES static Compound obstacles: entries of the batch's obstacle table, each at a pose of the world's
 * own ("the obstacle table" below); canonical constraint order only.  There are no bodies of more than four components, no moving obstacles,
 * no ghosts or tiles and no constraint_order = demo: a batch has no entry point for them.  A tick never fails for list sizes: a world whose
 * constraints outgrow its share of the storage gets its tick undone on the device and run again with more (Solver::solve and
 * World::step have no capacity failure, solver.rs:72-78); mgf_batch_counter "capacity_retries" counts those re-runs.
 * Calls are synchronous on the context's stream; the handle keeps a reference on the context; there is no CPU fallback.
 * PART QUERIES: mgf_batch_set_option(b, "part_queries", 1) (default 0: the refusals above stay) makes the calls that read shapes see
 * the parts of bodies of several components, on a batch that holds such bodies (without them the option changes no launch).  IN
 * SCOPE: mgf_batch_raycast_many(_dev), _sweep_many(_dev), _cast_sensors(_dev), _cast_feelers(_dev), _overlap_aabb_many,
 * _overlap_first_dev, _overlap_nearest_dev, _read_zones(_dev), _read_zones_nearest(_dev).  Each answers for world k, bit for bit, what
 * the lone mgf_world answers that has been through the same add calls and ticks: a ray tests every part of every body not ignored
 * (Intersects<Sphere | Capsule>), ranked (t, kind, index, part) ascending, and `part` of the hit is the part's index (0 for an ordinary
 * body); a sweep tests every part, ranked (t, kind, index, part, order emitted); a body's box is BoundedBy<AABB> of its parts combined
 * in order (bounds.rs:113-130), which is what the box overlaps, the zones and overlap_first_dev test and whose centre the nearest
 * forms measure from; an ignored body - ignore_body, MGF_SENSOR_IGNORE_SELF, MGF_FEELER_IGNORE_SELF - is skipped with every part of it.
 * The rigs' definitions do not change: a sensor answers mgf_batch_raycast_many of the particle it forms, a feeler _sweep_many of its
 * cast, a zone the box overlap of its box; MGF_FEELER_OWN_SHAPE on a body of several components casts the collider row as
 * mgf_batch_read_colliders packs it - a radius-0 sphere at the centre of mass.  Between ticks the parts are those of the last tick, or
 * as added before any tick (as the colliders): mgf_batch_write_state and mgf_batch_set_many move no part.  A call makes the number of
 * launches it makes without the option.  OUT OF SCOPE: mgf_batch_cast_cameras(_dev) stay refused ("several components") with the
 * option set too - the tile cull over parts is not built. */
#define MGF_BATCH_MAX_BODIES 1024
MGF_API mgf_status mgf_batch_new(mgf_ctx* ctx, const mgf_params* params, int64_t n_worlds, mgf_batch** out);  /* n_worlds x World::new world.rs:160 */
MGF_API void mgf_batch_free(mgf_batch* b);
/* ---- the terrain table: a mesh per world.  World k behaves, bit for bit, as a lone mgf_world that holds world k's bodies and has had
 * mgf_world_set_terrain called with mesh terrain[k] after mgf_mesh_set_pos(pos[k]) - the tick's state, the constraint list with impulses
 * (Static{ center } of a terrain constraint is the world's mesh position, world.rs:247), the statistics, the queries below (a face index
 * is the mesh's own) - or as one without terrain.  What a world computes depends neither on the order of the table nor on which other
 * worlds share its mesh; the number of launches of a tick or a query does not depend on the table.
 * mgf_batch_add_terrain copies the mesh (its tree, vertices, faces and current position) behind the table's last entry and returns its
 * id: 0, 1, ...; no world changes.  A mesh with an empty tree is a valid entry that behaves as no terrain.
 * mgf_batch_set_world_terrain applies n assignments in order (a world named twice keeps the last): world[i] gets entry terrain[i], or
 * none for -1, at pos[i], or with pos = NULL at the position the mesh had when it was added - one heightfield at a thousand offsets is
 * stored once.  It may be called between any two mgf_batch_step calls and holds from the next tick; it moves no body, no fat box and no
 * collider a query sees.
 * mgf_batch_terrain_count: the table's length, -1 for NULL.
 * mgf_batch_set_terrain(b, mesh) empties the table, makes `mesh` its entry 0 and gives it to every world at the mesh's position; with
 * NULL the table is empty and no world has terrain.
 * Refused with MGF_ERR_INVALID, nothing changed at all: a NULL batch, a NULL mesh or id, NULL world or terrain with n > 0, a negative n,
 * a world index outside [0, n_worlds), a terrain id below -1 or >= the table's length. */
MGF_API mgf_status mgf_batch_set_terrain(mgf_batch* b, const mgf_mesh* mesh);                     /* World.terrain, of every world */
MGF_API mgf_status mgf_batch_add_terrain(mgf_batch* b, const mgf_mesh* mesh, int32_t* id);
MGF_API mgf_status mgf_batch_set_world_terrain(mgf_batch* b, const int32_t* world, const int32_t* terrain, const mgf_vec3* pos, int64_t n);
MGF_API int64_t mgf_batch_terrain_count(const mgf_batch* b);
/* ---- the obstacle table: static Compound obstacles per world.  World k behaves, bit for bit, as a lone mgf_world that holds world k's
 * bodies, has world k's terrain at world k's mesh position, and has had mgf_world_add_obstacle called once per entry of world k's
 * obstacle list, in list order, each after mgf_compound_set_pose(disp, rot) with that entry's pose - the tick's state, the constraint
 * list with its impulses, the statistics (n_terrain_constraints counts obstacle contacts too) and the queries below.  The definition
 * is the lone world's (the oracle's World::obstacles): behind body i's terrain contacts every obstacle in list order goes through
 * Compound::contacts(&Moving::sweep(collider_i, delta_i)) (compound.rs:334-352), every contact a constraint of its own against
 * Static{ center: the entry's disp, friction: 0 }; the partners j < i follow.  What a world computes depends neither on the order of
 * the table, nor on which other worlds use the same entry, nor on where in the batch the world sits.
 * mgf_batch_add_obstacle copies the compound (components, tree and current pose) behind the table's last entry and returns its id: 0,
 * 1, ...; no world changes.  An empty compound is a valid entry that meets nothing but keeps its place in a world's list (a hit's
 * `index` still counts it; mgf_world_add_obstacle accepts one too).  A compound of 2^18 components or more: MGF_ERR_CAPACITY, as
 * mgf_world_add_obstacle.
 * mgf_batch_set_world_obstacles: every world some record names gets its list replaced by its records, in array order; a world no
 * record names is untouched.  A record with obstacle[i] = -1 contributes nothing: a world named only by such records ends with an
 * empty list.  disp and rot are per record; NULL (each on its own) means the pose the compound had when it was added; rot is taken
 * as normalised, as by mgf_compound_set_pose.  It may be called between any two mgf_batch_step calls and holds from the next tick; it
 * moves no body, no fat box, no collider and no constraint list.
 * mgf_batch_obstacle_count: the table's length, -1 for NULL.  mgf_batch_world_obstacle_count: the length of a world's list, -1 for a
 * NULL batch or a world index outside [0, n_worlds).
 * Refused with MGF_ERR_INVALID, nothing changed at all: a NULL batch, a NULL compound or id, NULL world or obstacle with n > 0, a
 * negative n, a world index outside [0, n_worlds), an id below -1 or >= the table's length, a world that would get more than
 * MGF_BATCH_MAX_WORLD_OBSTACLES entries.  The number of launches of a tick does not depend on the table or the lists. */
#define MGF_BATCH_MAX_WORLD_OBSTACLES 64
MGF_API mgf_status mgf_batch_add_obstacle(mgf_batch* b, const mgf_compound* c, int32_t* id);
MGF_API mgf_status mgf_batch_set_world_obstacles(mgf_batch* b, const int32_t* world, const int32_t* obstacle, const mgf_vec3* disp,
                                                 const mgf_quat* rot, int64_t n);
MGF_API int64_t mgf_batch_obstacle_count(const mgf_batch* b);                       /* the table's length; -1 for NULL */
MGF_API int64_t mgf_batch_world_obstacle_count(const mgf_batch* b, int64_t world);  /* a world's list; -1 for a bad argument */
/* World::add_body / RigidBodyVec::add_body (physics.rs:200-218, world.rs:178-184) in bulk, for world `world`; *first_id = the index of the
 * first new body within that world.  A tag other than 0 or 1, a negative n, a world index out of range: MGF_ERR_INVALID. */
MGF_API mgf_status mgf_batch_add_bodies(mgf_batch* b, int64_t world, const mgf_component* comps, int64_t n, const float* mass,
                                        const float* restitution, const float* friction, const mgf_vec3* world_force, uint64_t* first_id);
/* Bodies of 1..4 components for world `world`, as mgf_world_add_compound_bodies: body r is comps[offsets[r] .. offsets[r + 1]) in world
 * coordinates at creation, comp_mass per component, restitution / friction / world_force per body; mass = the sum, x = the centre of
 * mass, q = identity, parts fixed in the body frame and rebuilt from (x, q) every tick.  World k then behaves, bit for bit, as a lone
 * mgf_world that has been through the same mgf_world_add_bodies / mgf_world_add_compound_bodies calls in the same order (the oracle's
 * World::collide: a body's tight box is the union of its parts' swept bounds; per face met by that box the parts in order; per obstacle
 * the parts in order, each with its own query box; all part pairs of a pair of bodies - the first body's parts outer - through
 * ContactPruner and Manifold::from, every contact of the manifold a consecutive record with the manifold's normal, at most 16).
 * *first_id = the index of the first new body within that world; indices follow call order across mgf_batch_add_bodies and this call.
 * A body of ONE component is the ordinary body mgf_batch_add_bodies adds, with that component's mass; a batch without a body of more
 * than one component keeps no part storage and runs the tick it always ran.  Allowed behind ticks and into a world in the middle of
 * the batch; rigs keep naming the (world, body) they named.  mgf_batch_read_colliders gives such a body the lone world's row (a
 * radius-0 sphere at the centre of mass); mgf_batch_copy_worlds(_where) carry a world's part rows - the destination is a clone.
 * MGF_ERR_INVALID, nothing added, before the batch or a device is looked at: a NULL batch, comps, offsets or first_id; a negative n or
 * world; offsets[0] != 0; a body of 0 or of more than 4 components (the batch takes four, the lone world 32); a tag other than 0 or 1;
 * n > MGF_BATCH_MAX_BODIES.  A world index >= n_worlds or a world that would pass MGF_BATCH_MAX_BODIES: MGF_ERR_INVALID, nothing added.
 * A singular mass: MGF_ERR_SINGULAR. */
MGF_API mgf_status mgf_batch_add_compound_bodies(mgf_batch* b, int64_t world, const mgf_component* comps, const float* comp_mass,
                                                 const int64_t* offsets /* n + 1 */, int64_t n, const float* restitution,
                                                 const float* friction, const mgf_vec3* world_force, uint64_t* first_id);
MGF_API int64_t mgf_batch_len(const mgf_batch* b, int64_t world);   /* RigidBodyVec::len; world = -1: all bodies of the batch; -1 for a bad argument */
/* n_ticks x World::step (world.rs:227-294) of every world.  stats: NULL or n_ticks * n_worlds records, tick-major (record t * n_worlds + k =
 * world k's tick t): n_bodies, n_constraints, n_terrain_constraints, n_pair_candidates, n_refits and iters are filled; the fields the batch
 * path has no meaning for - n_terrain_candidates, n_levels, the ms_* times, solver_kernel_launches, n_ghost_constraints - are zero. */
MGF_API mgf_status mgf_batch_step(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, mgf_step_stats* stats);
/* As mgf_world_read_state / mgf_world_write_state (physics.rs:142-154) for world `world`, or for world = -1 the whole batch, worlds
 * concatenated in order; any array pointer may be NULL.  Writing one world's state between ticks resets that environment: no other
 * world is touched. */
MGF_API mgf_status mgf_batch_read_state(mgf_batch* b, int64_t world, mgf_vec3* x, mgf_quat* q, mgf_vec3* v, mgf_vec3* omega, mgf_vec3* delta, int64_t cap);
MGF_API mgf_status mgf_batch_write_state(mgf_batch* b, int64_t world, const mgf_vec3* x, const mgf_quat* q, const mgf_vec3* v, const mgf_vec3* omega,
                                         const mgf_vec3* delta, int64_t n);
/* The Solver's constraint list (solver.rs:53-79) of world `world`'s last tick, in insertion order; bodies by their index within the world. */
MGF_API mgf_status mgf_batch_read_constraints(mgf_batch* b, int64_t world, mgf_constraint* out, int64_t cap, int64_t* count);
/* ---- queries against the worlds of a batch, between ticks.  The definition is the lone world's ("queries against the world between
 * ticks", above): out[i] is, bit for bit, what mgf_world_raycast_many / mgf_world_sweep_many reports for query i on a lone mgf_world
 * that holds world world[i]'s bodies, that world's terrain at that world's mesh position (the terrain table, above) and that world's
 * obstacles at their poses (the obstacle table, above), and has been through the same calls.
 *   Ray cast: the closest hit of Intersects<shape> (collision.rs:169-373; compound.rs:150 for a component), the smallest t, ties to the
 *   target first in the order bodies (ascending index), terrain faces (ascending index), obstacles (Intersects<Compound>,
 *   compound.rs:309-332; ascending place in the world's list); a particle with d = 0 or with max|d_k| outside [MGF_RAY_DMIN,
 *   MGF_RAY_DMAX] hits nothing, and a hit whose t is not finite is not a candidate (mgf_world_raycast_many: one predicate serves both).
 *   Sweep: the earliest contact of Contacts<Moving<Sphere | Capsule>> of a body's sphere or capsule (collision.rs:1089-1356; :1143
 *   through commute_contacts!) and of Contacts<Moving<_>> for Poly of each face (collision.rs:610-1000, up to two contacts for a
 *   capsule) and of Compound::contacts of the cast for each obstacle (compound.rs:334-352), the least (t, kind, index, part, order
 *   emitted within the target); a contact whose t is not finite is not a candidate
 *   (collision.rs:693-1086); a capsule cast with delta = 0 tests every face (:901-1060), a capsule reaches max(1, |d|) (:698-719);
 *   delta = 0 is a valid cast (sphere on sphere with equal centres reports nothing, :1097-1100).
 * index is the body's index within its world, the face index, or (kind = MGF_HIT_OBSTACLE) the obstacle's place in the world's list;
 * part is 0, or the component of the obstacle.  ignore_body: NULL, or n indices within world world[i] (-1: none).  kinds_mask:
 * MGF_QUERY_* bits; 0 or a bit beyond MGF_QUERY_ALL is refused; MGF_QUERY_OBSTACLES matches the world's obstacles exactly as on the
 * lone world (one more launch, and only where the mask has the bit and some world of the batch has an obstacle).
 * The collider a query sees is the one the world's query would see: the one the last tick built (physics.rs:243-251); for a body no
 * tick has touched, the component it was added as; mgf_batch_write_state does not move it, as mgf_world_write_state does not.
 * mgf_batch_read_colliders returns exactly that collider with the body's current delta (colliders() physics.rs:256).
 * Refused with MGF_ERR_INVALID, nothing computed: a NULL batch, NULL arrays with n > 0, a negative n, a cast tag other than 0 or 1, a
 * world index < 0 or >= n_worlds, n > INT32_MAX.
 * out[i] depends on nothing but query i and world world[i] - not on the other queries, their order, or what else the batch holds.  A
 * query touches nothing of the tick's state: a step after a query is bit-identical to one without it.  The number of kernel launches
 * of a call depends on neither n_worlds nor n (mgf_batch_counter "query_launches"). */
/* As mgf_world_read_colliders for world `world`, or for world = -1 the whole batch, worlds concatenated in order. */
MGF_API mgf_status mgf_batch_read_colliders(mgf_batch* b, int64_t world, mgf_moving_component* out, int64_t cap);
/* n queries, query i against world world[i] (any order, any mix; a world may get none). */
MGF_API mgf_status mgf_batch_raycast_many(mgf_batch* b, const int32_t* world, const mgf_particle* parts, int64_t n,
                                          const int32_t* ignore_body, int32_t kinds_mask, mgf_ray_hit* out);
MGF_API mgf_status mgf_batch_sweep_many(mgf_batch* b, const int32_t* world, const mgf_moving_component* casts, int64_t n,
                                        const int32_t* ignore_body, int32_t kinds_mask, mgf_sweep_hit* out);
/* ---- what a caller reads of a batch every tick besides rays and sweeps: who touches what and how hard, who is in this box ----
 * mgf_batch_read_body_contacts: the constraint list of the last tick folded per body, on the device, beside the list.  The struct and
 * its definition are this build's: the reference has no such report (its Solver keeps the list, solver.rs:53-79, and World::step fills
 * it, world.rs:243-291; nothing there sums it per body).  The list described is exactly the one mgf_batch_read_constraints would return
 * for that world at that moment: the last tick's, in insertion order; empty before the first tick and, for every world, once bodies have
 * been added behind a tick; unchanged by mgf_batch_write_state.  Per body x, over the records that name x in the order of its chain -
 * its own range of the list first (x is `a`), then the records where x is `b`, ascending: the order ContactConstraint::solve
 * (solver.rs:203-252) meets them in - with impulse and normal_impulse starting at +0 and t = (normal.x * ni, normal.y * ni,
 * normal.z * ni), ni = the record's normal_impulse, in f32:  x is `a`: impulse = impulse - t (va -= impulse * inv_mass_a,
 * solver.rs:243-247); x is `b`: impulse = impulse + t; in both roles normal_impulse = normal_impulse + ni.  Sequential f32
 * operations in that order, no fused multiply-add: the answer is defined to the bit, and a body in no record gets an all-zero record.
 * Tangent impulses are not part of it: mgf_constraint does not carry them.  A record against an obstacle of the world counts in
 * n_terrain like every other record with b = -1. */
typedef struct mgf_body_contacts {
  int32_t n_contacts;     /* records of the list that name the body, as a or as b */
  int32_t n_terrain;      /* of those, records against RigidBodyRef::Static (b = -1; the body is a): terrain and obstacle contacts alike */
  mgf_vec3 impulse;       /* net accumulated normal impulse on the body, see above */
  float normal_impulse;   /* sum of the records' normal_impulse */
} mgf_body_contacts;      /* 24 bytes */
/* world: one world, or -1 for the whole batch, worlds concatenated in order (as mgf_batch_read_state); cap: records `out` holds.
 * MGF_ERR_INVALID: a NULL batch, NULL out, a world index < -1 or >= n_worlds; MGF_ERR_CAPACITY: cap below the number of bodies.
 * One kernel launch whatever the number of worlds and bodies, one copy, one host wait (counters "query_launches", "query_run_ns"). */
MGF_API mgf_status mgf_batch_read_body_contacts(mgf_batch* b, int64_t world, mgf_body_contacts* out, int64_t cap);
/* Box overlap, as mgf_world_overlap_aabb_many: box i against world world[i] (any order, any mix) reports every body of that world whose
 * tight bound BoundedBy<AABB> (bounds.rs:170-190) of the collider a query sees (above) passes Overlaps<AABB> (collision.rs:22-29),
 * in ascending body index within the world, at out_bodies[out_offsets[i] .. out_offsets[i+1]) - bit for bit what
 * mgf_world_overlap_aabb_many reports on a lone world with that world's bodies after the same calls.  A box with a NaN or a negative
 * half extent answers as the single test does.  out_offsets and *total are always filled; MGF_ERR_CAPACITY if *total > cap.
 * Refused with MGF_ERR_INVALID: a NULL batch, NULL arrays with n > 0, NULL out_offsets, a negative n or cap, a world index < 0 or
 * >= n_worlds, n > INT32_MAX.  The kernel launches of a call depend on neither n_worlds nor n ("query_launches": the collider gather
 * behind a step, count, fill; the prefix sum between them is the library's). */
MGF_API mgf_status mgf_batch_overlap_aabb_many(mgf_batch* b, const int32_t* world, const mgf_aabb* boxes, int64_t n,
                                               uint64_t* out_offsets /* n+1 */, uint32_t* out_bodies, int64_t cap, int64_t* total);
/* ---- driving a batch between ticks: get / set, forces and torques, impulses, world-to-world copies - on the device ----
 * A (world[i], body[i]) pair names body body[i] of world world[i]; any order, any mix of worlds, a world may get no record (the
 * addressing of mgf_batch_raycast_many).  The calls address a body no tick has touched yet like any other: a batch still in its host
 * mirror, bodies added behind a tick; for such a body inv_moment is inv_moment_body, as add_body leaves it (physics.rs:212-214).
 * They write the rows the tick reads - velocities, force, torque - and nothing else of the tick's state: fat boxes, colliders and the
 * constraint list stay as they are, mgf_batch_read_body_contacts / _read_constraints still describe the last tick and the collider a
 * query sees does not move, as mgf_world_set leaves the lone world.  A world that no record names is bit-for-bit untouched.
 * Forces and torques are rows of the body: they survive mgf_batch_add_bodies behind a tick, mgf_batch_write_state does not touch them,
 * mgf_batch_copy_worlds copies them.
 * Records that name the same body are resolved deterministically: the record indices are sorted by body on the host (a stable sort:
 * a body's records keep the caller's order) and one lane takes each body - no float atomic, no race between lanes.
 * The number of kernel launches of a call depends on neither n nor n_worlds (mgf_batch_counter "drive_launches").
 * Refused with MGF_ERR_INVALID, nothing changed: a NULL batch, NULL world / body with n > 0, NULL vel for mgf_batch_set_many, a negative
 * n or n > INT32_MAX, a world index outside [0, n_worlds), a body index outside [0, mgf_batch_len(b, world[i])).
 * OUT OF SCOPE here: the lone mgf_world gets no force setter (its migrant records, 148 floats and part of the ABI, carry the force but
 * no torque); impulses at a point; a whole-batch clone; copies between contexts. */
/* ConstrainedSet::get (physics.rs:272-304) for n bodies; any output may be NULL.  force / torque: RigidBodyVec.force / .torque
 * (physics.rs:146-147) as stored: force = world_force * mass at add_body (physics.rs:207). */
MGF_API mgf_status mgf_batch_get_many(mgf_batch* b, const int32_t* world, const int32_t* body, int64_t n,
                                      mgf_velocity* vel, mgf_rigid_body_info* info, mgf_vec3* force, mgf_vec3* torque);
/* ConstrainedSet::set (physics.rs:306-314), as n calls in array order: a body named twice keeps the last. */
MGF_API mgf_status mgf_batch_set_many(mgf_batch* b, const int32_t* world, const int32_t* body, int64_t n, const mgf_velocity* vel);
/* RigidBodyVec.force[i] = force[k], .torque[i] = torque[k]; either array NULL = left as it is; a body named twice keeps the last.
 * Holds for every later tick until set again (physics.rs:236, 240 read them every integrate). */
MGF_API mgf_status mgf_batch_set_forces(mgf_batch* b, const int32_t* world, const int32_t* body, int64_t n,
                                        const mgf_vec3* force, const mgf_vec3* torque);
/* This build's definition (the reference changes velocities only inside ContactConstraint::solve, solver.rs:243-247, in this form):
 * record k, in array order:  v = v + linear[k] * inv_mass;  omega = omega + I * angular[k]
 * inv_mass and I = the world-frame inv_moment as mgf_batch_get_many returns them at that moment.
 * M * v = (c0 * v.x + c1 * v.y) + c2 * v.z (cgmath, column-major).  f32, no fused multiply-add.
 * A body named several times receives its records one after the other in array order: the answer is defined to the bit.
 * Either array NULL = zero for all records of that array. */
MGF_API mgf_status mgf_batch_apply_impulses(mgf_batch* b, const int32_t* world, const int32_t* body, int64_t n,
                                            const mgf_vec3* linear, const mgf_vec3* angular);
/* RigidBodyVec: Clone (physics.rs:140) per world: world dst_world[i] of dst becomes world src_world[i] of src.  dst and src are one batch
 * or two batches of one context.  src is const in what it holds, not in where: a source batch that is still in its host mirror is
 * moved to the device first (its bodies, shares and lists allotted as its own next call would), nothing of its state changes.
 * Copied is everything that makes the world step on, and answer, exactly like its source: every
 * persistent row of its bodies (state, velocities, inverse mass and inertias, force, torque, restitution, friction, constructor, delta,
 * fat box, the collider a query sees), the tick's packed copy, and the last tick's constraint list with its impulses and its length -
 * mgf_batch_read_constraints, _read_body_contacts, _read_colliders, the ray casts, sweeps and box overlaps answer for the destination
 * what they answer for the source, and with the same terrain the destination steps bit-identically to the source.
 * Not copied: the terrain assignment and the obstacle list (the environment is the destination's: mgf_batch_set_world_terrain and
 * mgf_batch_set_world_obstacles copy them; with the same terrain and the same list the destination steps like the source), the shares of the
 * storage (a destination whose share is smaller than the source's list gets a larger one first, and keeps it - as a world keeps
 * what a tick that did not fit asked for - until "cons_per_body" is set again), counters and options.
 * A source may be named any number of times (fan-out).  Refused with MGF_ERR_INVALID, nothing copied, before any launch: a NULL batch,
 * NULL arrays with n > 0, a negative n or n > INT32_MAX, a world index out of range, batches of different contexts, a destination and
 * its source of different lengths, a destination named twice, and - where dst == src - a world that is both a source and a
 * destination.  One workgroup per pair, one launch (and one more when shares grow): "drive_launches" of dst.
 * Bodies of several components: a world's part rows travel in one more launch - the destination is a clone.  When src holds part
 * storage (it has held a body of more than one component) and dst does not, dst gets it before anything is enqueued and KEEPS it,
 * whatever the copied worlds hold: from then on dst ticks in seven launches and its calls that read the shapes of bodies (ray casts,
 * sweeps, box overlaps, sensors, cameras, zones) return MGF_ERR_INVALID ("several components"), as on src. */
MGF_API mgf_status mgf_batch_copy_worlds(mgf_batch* dst, const int32_t* dst_world, const mgf_batch* src, const int32_t* src_world, int64_t n);
/* ---- device-pointer calls: state, forces, impulses, contact summaries and resets for a caller whose arrays are device memory ----
 * The calls above move their records through host memory (an upload or a download and a host wait per call).  These take pointers
 * marked *_dev* / documented as device memory: memory of the context's device (hipMalloc or managed - e.g. a torch tensor's data_ptr()).
 * Each call is enqueued on the context's stream and RETURNS WITHOUT WAITING for it: order the caller's own work against it with
 * mgf_ctx_set_stream (one shared stream) or wait with mgf_ctx_synchronize.  In the steady state - the batch on the device, the handle's
 * scratch buffers large enough, and for the masked copy an unchanged pair table - a call makes no host wait and no copy between host
 * and device.
 * A body is named by its flat index g = (bodies in the worlds before its world) + index within its world: the order of
 * mgf_batch_read_state(world = -1).  body_dev == NULL: record i names body i, and n <= mgf_batch_len(b, -1).
 * Every index is checked on the device: a record whose index lies outside [0, mgf_batch_len(b, -1)) is skipped whole - it reads nothing
 * and writes nothing - and counted in mgf_batch_counter "device_skipped" (cumulative over the batch's life; reading it waits for the
 * stream).
 * Pointer safety: before anything is enqueued every non-NULL device pointer is looked up on the host - hipPointerGetAttributes must
 * report device or managed memory of the context's device, hipMemGetAddressRange that the bytes the call will touch lie inside the
 * allocation - and the pointer must be 4-byte aligned; else MGF_ERR_INVALID, nothing enqueued.  Also refused before any device work: a
 * NULL batch, a negative n, n > INT32_MAX, and what each call names below.
 * Launches ("drive_launches" of the batch, as for the host-memory calls; none depends on n or on n_worlds):
 *   mgf_batch_gather_state_dev                     1
 *   the three setters, body_dev == NULL            1
 *   the three setters, body_dev given              MGF_BATCH_DEV_SET_LAUNCHES = 3 (count, fill, apply; the prefix sum between count and
 *                                                  fill is the library's and is not counted, as for mgf_batch_overlap_aabb_many)
 *   mgf_batch_copy_worlds_where                    1, and 1 more when shares grow (as mgf_batch_copy_worlds)
 *   mgf_batch_read_body_contacts_dev               1 ("query_launches", as mgf_batch_read_body_contacts)
 *   mgf_batch_raycast_many_dev / _sweep_many_dev   "query_launches": the collider gather behind a step (1, once), then with world_dev
 *                                                  given MGF_BATCH_DEV_QUERY_PLAN_LAUNCHES = 3 (count, cut, fill; the two prefix sums
 *                                                  between cut and fill are the library's and are not counted), with world_dev == NULL
 *                                                  0; then the passes of the host-memory call: bodies 1, a sweep's faces 1 where the
 *                                                  mask asks for terrain and a world has one, obstacles 1 where the mask asks for them
 *                                                  and a world has one
 *   mgf_batch_cast_sensors / _cast_sensors_dev     "query_launches": the collider gather behind a step (1, once), then
 *                                                  MGF_BATCH_SENSOR_LAUNCHES = 1, and obstacles 1 where the mask asks for them and a
 *                                                  world has one
 * OUT OF SCOPE here: device-pointer box queries (their CSR total needs a host wait - a record of fixed width per box needs none:
 * mgf_batch_read_zones_dev / mgf_batch_overlap_first_dev, below); rays given in a body's frame per call (a rig that is
 * set once has mgf_batch_set_sensors / _cast_sensors_dev, below); a step without its
 * one host wait per call (the capacity re-runs need it); hipGraph capture of these calls; anything for the lone mgf_world (it has
 * mgf_world_export_bodies / _import_ghosts / _device_ptr). */
#define MGF_BATCH_DEV_SET_LAUNCHES 3
#define MGF_BATCH_DEV_QUERY_PLAN_LAUNCHES 3
/* Tightly packed rows for record i: 3 floats, 4 for q (s, x, y, z: mgf_quat).  Any output may be NULL.  x, v, omega, force, torque
 * equal mgf_batch_get_many's for the same bodies bit for bit (x is x + delta, physics.rs:282), q equals mgf_batch_read_state's. */
MGF_API mgf_status mgf_batch_gather_state_dev(mgf_batch* b, const int32_t* body_dev, int64_t n,
                                              float* x, float* q, float* v, float* omega, float* force, float* torque);
/* mgf_batch_set_many / _set_forces / _apply_impulses with rows of 3 floats in device memory: the same rows written, the same left alone.
 * linear and angular of mgf_batch_set_many_dev are both required (NULL: MGF_ERR_INVALID); either array of the other two may be NULL
 * (force / torque: that row is left as it is; linear / angular: zero for every record).
 * Records that name the same body are resolved on the device, to the definition of the host path's stable sort: a set takes the record
 * with the highest array index; an impulse run is applied in ascending array index, v = v + linear * inv_mass, omega = omega + I *
 * angular, sequential f32 operations, no fused multiply-add.  One lane owns a body, there is no float atomic, nothing of the answer
 * depends on lane scheduling.  (The lane orders a body's records by insertion: a call that names ONE body many thousands of times is
 * slow, not wrong.)  The caller's arrays must not change until the call has run. */
MGF_API mgf_status mgf_batch_set_many_dev(mgf_batch* b, const int32_t* body_dev, int64_t n, const float* linear, const float* angular);
MGF_API mgf_status mgf_batch_set_forces_dev(mgf_batch* b, const int32_t* body_dev, int64_t n, const float* force, const float* torque);
MGF_API mgf_status mgf_batch_apply_impulses_dev(mgf_batch* b, const int32_t* body_dev, int64_t n, const float* linear, const float* angular);
/* mgf_batch_read_body_contacts written straight into the caller's device buffer of cap records: no copy, no wait; "query_run_ns" is 0. */
MGF_API mgf_status mgf_batch_read_body_contacts_dev(mgf_batch* b, int64_t world, mgf_body_contacts* out_dev, int64_t cap);
/* mgf_batch_copy_worlds for the pairs a mask in device memory selects: pair i is copied iff mask_dev[i] != 0 (read by the pair's
 * workgroup); a copied pair is bit-identical to mgf_batch_copy_worlds of that pair, a masked-out destination is untouched to the bit.
 * dst_world and src_world are HOST arrays, checked and refused exactly as mgf_batch_copy_worlds does; also refused: NULL mask_dev with
 * n > 0.  The host cannot know the mask: the share of EVERY named destination grows to its source's list before the launch (a larger
 * share than needed may stay; no record is lost).  The pair table stays on the device in dst and is uploaded again only when the arrays
 * differ from the last call's (mgf_batch_counter "pair_table_uploads", cumulative).  mgf_batch_read_constraints and a later copy out of
 * dst first fetch the lengths of dst's lists from the device (one wait); mgf_batch_step does that anyway.
 * As mgf_batch_copy_worlds, a src with part storage makes dst a batch with part storage for good - also when the mask selects nothing:
 * the host cannot know the mask.  A ray cast on dst that then returns MGF_ERR_INVALID ("several components") has this cause. */
MGF_API mgf_status mgf_batch_copy_worlds_where(mgf_batch* dst, const int32_t* dst_world, const mgf_batch* src, const int32_t* src_world,
                                               int64_t n, const int32_t* mask_dev);
/* Of a batch's rays, sweeps and box queries the first two have a device-pointer form, the observations a policy reads every tick.
 * mgf_batch_raycast_many / mgf_batch_sweep_many with every array in device memory: out_dev[i] is, bit for bit, what the host-memory
 * call writes to out[i] for the same query, world, ignore entry and mask on the same batch at the same moment - every kind bit, terrain
 * table, obstacle list and "the collider a query sees" (above).  Nothing of the tick's state is written.  Enqueued on the context's
 * stream, not waited for; in the steady state - the batch on the device, the terrain and obstacle tables unchanged, the handle's scratch
 * large enough - no host wait and no copy between host and device.  No HIP events: "query_run_ns" is 0.
 * The sort by world is built on the device (ranks within a world by integer atomics, the library's prefix sums, work items of up to 256
 * queries).  The order of a world's queries inside a work item then depends on lane scheduling; no answer depends on that order, and
 * every answer is stored by the caller's index.  No float atomic.
 * world_dev == NULL is the fixed sensor layout: n must be a multiple of n_worlds (else MGF_ERR_INVALID), query i belongs to world
 * i / (n / n_worlds); no sort, no plan, nothing uploaded.
 * Checked on the device, before the index reads anything: a record whose world_dev[i] lies outside [0, n_worlds) - for a cast also one
 * whose tag is neither 0 nor 1 - is skipped whole: matched against nothing, out_dev[i] = the no-hit record (kind MGF_HIT_NONE, every
 * other word zero), counted in "device_skipped".  ignore_body_dev[i] (NULL: none) is only ever compared with a body index: a value that
 * is no body of that world ignores nothing.
 * Refused with MGF_ERR_INVALID, nothing enqueued: a NULL batch, a negative n or n > INT32_MAX, NULL parts_dev / casts_dev / out_dev with
 * n > 0, a mask of 0 or with bits beyond MGF_QUERY_ALL, a pointer that fails the look-up above (world_dev and ignore_body_dev 4 n bytes,
 * parts_dev 28 n, casts_dev 44 n, out_dev 28 n / 52 n), and out_dev's bytes overlapping those of an input array (a later pass reads the
 * queries again after an earlier one wrote hits).  The caller's arrays must not change until the call has run. */
MGF_API mgf_status mgf_batch_raycast_many_dev(mgf_batch* b, const int32_t* world_dev, const mgf_particle* parts_dev, int64_t n,
                                              const int32_t* ignore_body_dev, int32_t kinds_mask, mgf_ray_hit* out_dev);
MGF_API mgf_status mgf_batch_sweep_many_dev(mgf_batch* b, const int32_t* world_dev, const mgf_moving_component* casts_dev, int64_t n,
                                            const int32_t* ignore_body_dev, int32_t kinds_mask, mgf_sweep_hit* out_dev);
/* ---- body-mounted ray sensors: rays fixed in the frame of a body, cast from the poses resident on the device in one call ----
 * A range finder, a whisker, a ground probe, a line-of-sight check: a ray that is fixed in the frame of a body and moves with it.  A
 * sensor is a record (world, body, p, d, dt, flags): body an index within world, p and d in the body's frame.  With x and q the body's
 * rows as mgf_batch_read_state returns them - x WITHOUT delta: the pose from which the last tick built the collider a query sees - the
 * sensor's particle in world coordinates is
 *     P = x + rotate(q, p)      D = rotate(q, d)      dt unchanged
 * rotate = Rotation::rotate_vector (Quaternion * Vector3: tmp = v x r + r * s; (v x tmp) * 2 + r, v and s the quaternion's vector and
 * scalar part), the sum a plain vector add, every operation a separate f32 one, no fused multiply-add: P and D are defined to the bit.
 * The sensor's answer is, bit for bit, what mgf_batch_raycast_many writes for the particle (P, D, dt) against world `world` with the
 * same mask and the ignore value `body` if flags & MGF_SENSOR_IGNORE_SELF, else -1.  Every rule of that call holds unchanged: D = 0
 * hits nothing, ties are resolved as there, the colliders are those the last tick built ("the collider a query sees", above), nothing
 * of the tick's state is touched - a step after a cast is bit-identical to one without it.
 * After a mgf_batch_write_state a sensor follows the new x and q AT ONCE; the colliders move at the next tick (mgf_batch_write_state
 * does not move the collider a query sees).  (mgf_batch_gather_state_dev's x is x + delta: a ray a caller builds from it does not start
 * where the collider stands; a sensor with p = 0 starts at the centre of its body's collider frame.)
 * A rig is static, so what depends on it alone is done once, by mgf_batch_set_sensors: the checks, the sort by world, the work items of
 * up to 256 sensors.  A cast is then MGF_BATCH_SENSOR_LAUNCHES = 1 launch (and the obstacle pass, and the collider gather behind a
 * step: "query_launches") whatever the number of sensors and worlds - no plan, no index arrays. */
#define MGF_SENSOR_IGNORE_SELF 1
#define MGF_BATCH_SENSOR_LAUNCHES 1
typedef struct mgf_batch_sensor { int32_t world, body; mgf_vec3 p, d; float dt; int32_t flags; } mgf_batch_sensor;  /* 40 bytes */
/* Replaces the rig by a copy of s[0 .. n); n = 0 clears it.  Checked on the host and refused with MGF_ERR_INVALID, the rig as it was: a
 * NULL batch, a NULL array with n > 0, a negative n or n > INT32_MAX, a world outside [0, n_worlds), a body outside
 * [0, mgf_batch_len(b, world)), a flag bit beyond MGF_SENSOR_IGNORE_SELF.  No device work: the rig goes up with the next cast.
 * The rig names (world, body), not flat indices: mgf_batch_add_bodies afterwards - also into a world in the middle of the batch -
 * leaves every sensor on the body it named. */
MGF_API mgf_status mgf_batch_set_sensors(mgf_batch* b, const mgf_batch_sensor* s, int64_t n);
/* the sensors of the rig; -1 for NULL */
MGF_API int64_t mgf_batch_sensor_count(const mgf_batch* b);
/* The hit of sensor i at out[i], in the order of the array mgf_batch_set_sensors was given; parts_out non-NULL: also its particle
 * (P, D, dt) at parts_out[i] - what turns t into a point, or draws the ray.  cap: records each array holds.
 * MGF_ERR_INVALID: a NULL batch, a negative cap, a mask of 0 or with bits beyond MGF_QUERY_ALL, NULL out with a rig that is not empty;
 * MGF_ERR_CAPACITY: cap below mgf_batch_sensor_count.  An empty rig: MGF_OK, nothing enqueued.  Synchronous, as mgf_batch_raycast_many: one download, one host
 * wait.  No HIP events: "query_run_ns" is 0. */
MGF_API mgf_status mgf_batch_cast_sensors(mgf_batch* b, int32_t kinds_mask, mgf_ray_hit* out, mgf_particle* parts_out, int64_t cap);
/* The same with both arrays in device memory (the device-pointer calls, above): enqueued on the context's stream and NOT waited for.  In
 * the steady state - the rig, the batch and the terrain and obstacle tables on the device, the handle's scratch large enough - no host
 * wait and no copy between host and device.  Also refused with MGF_ERR_INVALID, nothing enqueued: a pointer that fails the look-up of
 * the device-pointer calls (28 * count bytes each), and out_dev's bytes overlapping parts_out_dev's. */
MGF_API mgf_status mgf_batch_cast_sensors_dev(mgf_batch* b, int32_t kinds_mask, mgf_ray_hit* out_dev, mgf_particle* parts_out_dev, int64_t cap);
/* ---- body-mounted depth cameras: an image of rays fixed in the frame of a body, cast from the resident poses a tile at a time ----
 * An egocentric depth map, a height scan of the terrain under a walker, a lidar sweep: a pinhole camera fixed in the frame of a body.
 * Described pixel by pixel as sensors it would be a record of 40 bytes a pixel; a camera is one record of 64 bytes, and its kernel's
 * unit of work is an image tile, whose pixels settle together which bodies any of them can meet.
 * The camera looks along +z of its own frame, with +x to the right and +y up.  Pixel (ix, iy) sits at row iy from the top and column ix
 * from the left.  Its direction in the camera's frame is, in f32 with every operation rounded on its own and no fused multiply-add,
 *     u = ((float)(2*ix + 1) / (float)width  - 1.0f) * tan_x
 *     v = (1.0f - (float)(2*iy + 1) / (float)height) * tan_y
 *     d_cam = (u, v, 1.0f)
 * With x and q the body's rows as mgf_batch_read_state returns them (x WITHOUT delta, as for a sensor), the pixel's particle is
 *     P = x + rotate(q, p)      D = rotate(q, rotate(r, d_cam))      dt = far
 * rotate as in the sensors' definition above (Rotation::rotate_vector), r taken as given and not normalised.
 * The pixel's hit record is, bit for bit, what mgf_batch_raycast_many writes for the particle (P, D, far) against world `world` with the
 * call's mask and the ignore value `body` if flags & MGF_SENSOR_IGNORE_SELF, else -1.  The pixel's depth is the hit's inter.t, or far
 * where the kind is MGF_HIT_NONE.  d_cam.z is 1, so t IS the depth along the optical axis wherever r and q are unit quaternions (for
 * another r it is the hit's parameter along D, as for any ray).
 * Everything else is the sensors' text: the colliders are those the last tick built; after a mgf_batch_write_state a camera follows the
 * new x and q AT ONCE and its targets move at the next tick; a cast touches nothing of the tick's state - a step after a cast is bit-identical to
 * one without it.  Pixels come out camera by camera in the order of the array given, row-major within a camera: pixel (ix, iy) of
 * camera c at first(c) + iy * width + ix, first(c) the pixels of the cameras before c.
 * "query_launches" of a cast: the collider gather behind a step (1, once), then MGF_BATCH_CAMERA_LAUNCHES = 1; where the mask asks for
 * obstacles and a world has one, the unchanged obstacle pass over the stored particles and hit records (1; both live in the handle's
 * scratch when the caller gave no array) and a lane-per-pixel pass that writes depth from the final hits (1; not where depth is NULL).
 * None of it depends on the number of cameras, pixels or worlds.
 * OUT OF SCOPE here: a near plane; colour, or anything but depth and the hit; several small cameras sharing one workgroup (a camera of
 * a few pixels wastes lanes: a few rays are what sensors are for); a tile cull of the terrain walk; cameras on the lone mgf_world. */
#define MGF_BATCH_CAMERA_LAUNCHES 1
#define MGF_CAMERA_MAX_SIDE 4096
typedef struct mgf_batch_camera {
  int32_t world, body;     /* body: an index within world */
  mgf_vec3 p;              /* the eye, in the body's frame */
  mgf_quat r;              /* the camera's orientation in the body's frame (s, x, y, z); taken as given, not normalised */
  float tan_x, tan_y;      /* tangents of the half angles of view, horizontal and vertical */
  float far;               /* the rays' dt: > 0, or +inf */
  int32_t width, height;   /* pixels */
  int32_t flags;           /* MGF_SENSOR_IGNORE_SELF or 0 */
  int32_t reserved;        /* 0 */
} mgf_batch_camera;        /* 64 bytes */
/* Replaces the camera rig by a copy of cams[0 .. n); n = 0 clears it.  Checked on the host and refused with MGF_ERR_INVALID, the rig as
 * it was: what mgf_batch_set_sensors refuses (a NULL batch, a NULL array with n > 0, a negative n or n > INT32_MAX, a world or a body
 * out of range, a flag bit beyond MGF_SENSOR_IGNORE_SELF); a width or height outside [1, MGF_CAMERA_MAX_SIDE]; more than INT32_MAX pixels
 * in all; a non-finite p, r, tan_x or tan_y; a far that is NaN or <= 0; reserved != 0.  No device work: the rig - the records and a
 * table of its tiles - goes up with the next cast.  The rig is independent of the sensor rig: each can be set, cleared and cast without
 * the other changing.  It names (world, body): mgf_batch_add_bodies afterwards leaves every camera on the body it named. */
MGF_API mgf_status mgf_batch_set_cameras(mgf_batch* b, const mgf_batch_camera* cams, int64_t n);
/* the cameras of the rig, and the pixels of all of them; -1 for NULL */
MGF_API int64_t mgf_batch_camera_count(const mgf_batch* b);
MGF_API int64_t mgf_batch_camera_pixels(const mgf_batch* b);
/* depth: float[pixels], hits: mgf_ray_hit[pixels], parts_out: mgf_particle[pixels]; each may be NULL.  cap: records each array holds.
 * MGF_ERR_INVALID: a NULL batch, a negative cap, a mask of 0 or with bits beyond MGF_QUERY_ALL, depth and hits both NULL with a rig that
 * is not empty; MGF_ERR_CAPACITY: cap below mgf_batch_camera_pixels.  An empty rig: MGF_OK, nothing enqueued.  Synchronous, as
 * mgf_batch_cast_sensors: one download an array, one host wait.  No HIP events: "query_run_ns" is 0. */
MGF_API mgf_status mgf_batch_cast_cameras(mgf_batch* b, int32_t kinds_mask, float* depth, mgf_ray_hit* hits, mgf_particle* parts_out, int64_t cap);
/* The same with the arrays in device memory (the device-pointer calls, above): enqueued on the context's stream and NOT waited for.  In
 * the steady state - the rig, the batch and the terrain and obstacle tables on the device, the handle's scratch large enough - no host
 * wait and no copy between host and device.  Also refused with MGF_ERR_INVALID, nothing enqueued: a pointer that fails the look-up of
 * the device-pointer calls (4, 28 and 28 bytes a pixel), and any two of the three arrays overlapping. */
MGF_API mgf_status mgf_batch_cast_cameras_dev(mgf_batch* b, int32_t kinds_mask, float* depth_dev, mgf_ray_hit* hits_dev, mgf_particle* parts_out_dev,
                                              int64_t cap);
/* ---- box zones: who is in this box - the count and the first k bodies, a record of fixed width, answered on the device ----
 * A goal region, a pressure plate, a proximity volume round an agent, "the k bodies near me": an axis-aligned box whose centre is fixed
 * in the frame of a body, or in the world.  mgf_batch_overlap_aabb_many answers such a box in CSR form, whose total the caller must know
 * before it can size the lists: a host wait.  A policy reads an observation of fixed width; with a record of 1 + k words per box no
 * total is needed, count and fill are one pass, and nothing waits.
 * A zone is a record (world, body, p, r, flags, reserved): body an index within world, or -1 for a zone fixed in the world.  With x and q
 * the body's rows as mgf_batch_read_state returns them - x WITHOUT delta, as for a sensor - the zone's box is the mgf_aabb
 *     c = x + rotate(q, p)      r = r            (body = -1: c = p)
 * rotate and the add exactly the sensors' f32 operations (above): every operation rounded on its own, no fused multiply-add - c is
 * defined to the bit.  The box stays axis-aligned: only its centre rides on the body.  p and r are taken as given: a NaN or a negative
 * half extent answers as the single Overlaps<AABB> test does, as in mgf_batch_overlap_aabb_many (a NaN box holds nothing).
 * The record of a zone, for a call's k: let `list` be what mgf_batch_overlap_aabb_many reports for that box against `world` at that
 * moment - the bodies whose tight bounds of "the collider a query sees" (above) overlap it, in ascending body index - with `body` removed
 * if flags & MGF_SENSOR_IGNORE_SELF.  The record is 1 + k int32 words: word 0 is len(list), the full count, NOT truncated; words 1 .. k
 * are list[0 .. min(len, k)); the rest are -1.  Every word is defined to the bit.
 * After a mgf_batch_write_state a zone follows the new x and q AT ONCE; the colliders move at the next tick.  Nothing of the tick's state
 * is touched - a step after a read is bit-identical to one without it.
 * "query_launches" of a read: the collider gather behind a step (1, once), then MGF_BATCH_ZONE_LAUNCHES = 1, whatever the number of
 * worlds, zones and k.  No HIP events: "query_run_ns" is 0.
 * OUT OF SCOPE here: a world tensor for mgf_batch_overlap_first_dev; oriented boxes (the reference's Overlaps is AABB against AABB);
 * (nearest first: the next section, "box zones, nearest first"); zones on the lone mgf_world; a rig chosen per call by a device mask; hipGraph capture; terrain faces or
 * obstacles in a zone. */
#define MGF_BATCH_ZONE_LAUNCHES 1
typedef struct mgf_batch_zone { int32_t world, body; mgf_vec3 p, r; int32_t flags, reserved; } mgf_batch_zone;  /* 40 bytes */
/* Replaces the zone rig by a copy of z[0 .. n); n = 0 clears it.  Checked on the host and refused with MGF_ERR_INVALID, the rig as it
 * was: what mgf_batch_set_sensors refuses (a NULL batch, a NULL array with n > 0, a negative n or n > INT32_MAX, a world out of range, a
 * body >= mgf_batch_len(b, world), a flag bit beyond MGF_SENSOR_IGNORE_SELF); body < -1; body = -1 together with MGF_SENSOR_IGNORE_SELF;
 * reserved != 0.  No device work: the rig goes up with the next read.  It is independent of the sensor and camera rigs.  It names
 * (world, body): mgf_batch_add_bodies afterwards leaves every zone on the body it named. */
MGF_API mgf_status mgf_batch_set_zones(mgf_batch* b, const mgf_batch_zone* z, int64_t n);
/* the zones of the rig; -1 for NULL */
MGF_API int64_t mgf_batch_zone_count(const mgf_batch* b);
/* The record of zone i at out[(1 + k) * i], in the order of the array mgf_batch_set_zones was given; boxes_out non-NULL: also its box
 * (c, r) as formed at boxes_out[i].  cap: records each array holds.  MGF_ERR_INVALID: a NULL batch, k < 0 or k > MGF_BATCH_MAX_BODIES,
 * a negative cap, NULL out with a rig that is not empty; MGF_ERR_CAPACITY: cap below mgf_batch_zone_count.  An empty rig: MGF_OK, nothing
 * enqueued.  Synchronous: one download, one host wait. */
MGF_API mgf_status mgf_batch_read_zones(mgf_batch* b, int32_t k, int32_t* out, mgf_aabb* boxes_out, int64_t cap);
/* The same with both arrays in device memory (the device-pointer calls, above): enqueued on the context's stream and NOT waited for.  In
 * the steady state - the rig and the batch on the device - no host wait and no copy between host and device.  Also refused with
 * MGF_ERR_INVALID, nothing enqueued: a pointer that fails the look-up of the device-pointer calls (4 (1 + k) count and 24 count bytes),
 * and out_dev's bytes overlapping boxes_out_dev's. */
MGF_API mgf_status mgf_batch_read_zones_dev(mgf_batch* b, int32_t k, int32_t* out_dev, mgf_aabb* boxes_out_dev, int64_t cap);
/* The same kernel for boxes the caller computed on the device.  The fixed layout only: n must be a multiple of n_worlds (else
 * MGF_ERR_INVALID), box i is held against world i / (n / n_worlds); out_dev[(1 + k) * i ...] is the record of box i as defined above,
 * with ignore_body_dev[i] (NULL: none) removed from its list - only ever compared with a body index: a value that is no body of that
 * world removes nothing.  Refused with MGF_ERR_INVALID, nothing enqueued, in the order of mgf_batch_raycast_many_dev with
 * world_dev == NULL: a NULL batch, a negative n or n > INT32_MAX, NULL boxes_dev / out_dev with n > 0, k < 0 or k >
 * MGF_BATCH_MAX_BODIES, n no multiple of n_worlds, a pointer that fails the look-up (boxes_dev 24 n bytes, ignore_body_dev 4 n, out_dev
 * 4 (1 + k) n), out_dev's bytes overlapping those of an input array.  Not waited for; MGF_BATCH_ZONE_LAUNCHES = 1 launch. */
MGF_API mgf_status mgf_batch_overlap_first_dev(mgf_batch* b, const mgf_aabb* boxes_dev, int64_t n, const int32_t* ignore_body_dev, int32_t k,
                                               int32_t* out_dev);
/* ---- box zones, nearest first: the count and the k nearest bodies of every box, every word defined to the bit ----
 * Once a box holds more than k bodies, the first k in ascending index are an arbitrary subset of them.  "The k bodies near me" wants the
 * near ones, nearest first, and - for an observation - how far they are.  These are the zone rig's three reads (above) with that record;
 * the rig, mgf_batch_set_zones and every call above are unchanged.
 * A zone's box Q = (c, r) is formed exactly as above: c = x + rotate(q, p), and c = p for body = -1.  `list` is a zone's list as above:
 * what mgf_batch_overlap_aabb_many reports for Q against the zone's world, with the zone's own body removed if MGF_SENSOR_IGNORE_SELF
 * is set.  For body i of list let m_i be the centre of its tight box - the c of BoundedBy<AABB> (bounds.rs:170-188) of the collider a
 * query sees, the box the overlap test itself uses: a sphere's c; a capsule's a + d * 0.5.  With e = m_i - c the distance is
 *     d2_i = (e.x * e.x + e.y * e.y) + e.z * e.z
 * in f32, every operation rounded on its own, no fused multiply-add.  A listed body's d2 is never NaN (a NaN difference on any axis
 * fails Overlaps<AABB>: such a body is not in list); it lies in [+0, +inf], and f32 `<` on it is a total order.
 * The nearest record of a zone, for a call's k, is 1 + k int32 words: word 0 is len(list), the full count - the word
 * mgf_batch_read_zones writes; words 1 .. min(len, k) are the bodies of list in ascending (d2, body index); the rest are -1.  Where
 * asked for there are also k f32 words per zone: d2 of the listed bodies in the same order, then +INFINITY (0x7F800000) in every unused
 * word - a listed body whose d2 overflowed also reads +inf: the count says how many words are real.  Every word is defined to the bit:
 * it depends on neither the lanes a zone gets, nor the other zones of its work item, nor the rig's order.
 * 0 <= k <= MGF_BATCH_ZONE_NEAREST_MAX_K = 32: an observation of nearest neighbours is short, and the first-k record stays for anything
 * longer.  A NaN or negative box answers as the zones do (it holds nothing: count 0).  A zone follows mgf_batch_write_state AT ONCE, the
 * colliders move at the next tick, and nothing of the tick's state is touched, as above.  On a batch that holds bodies of several
 * components the three calls return MGF_ERR_INVALID ("several components"), as every call that reads shapes.
 * "query_launches" of a read: the collider gather behind a step (1, once), then MGF_BATCH_NEAREST_LAUNCHES = 1, whatever the number of
 * worlds, zones and k.  No HIP events: "query_run_ns" is 0.  The cost is 1 + ceil(k / 4) passes over a world's bodies, shared by a zone's
 * lanes.
 * OUT OF SCOPE here: the distance to a body's surface instead of its tight box's centre; terrain faces or obstacles in a zone; k above
 * 32; a world tensor for the fixed layout; zones on the lone mgf_world; hipGraph capture. */
#define MGF_BATCH_ZONE_NEAREST_MAX_K 32
#define MGF_BATCH_NEAREST_LAUNCHES 1
/* mgf_batch_read_zones with the nearest record: zone i's at out[(1 + k) * i], in the rig's order; dist2_out non-NULL: its k distances
 * at dist2_out[k * i]; boxes_out non-NULL: its box (c, r) as formed at boxes_out[i].  cap: records each array holds.  Refused as
 * mgf_batch_read_zones refuses, in its order - MGF_ERR_INVALID: a NULL batch, k < 0 or k > MGF_BATCH_ZONE_NEAREST_MAX_K ("k is outside
 * [0, MGF_BATCH_ZONE_NEAREST_MAX_K]", ahead of a negative cap), a negative cap, NULL out with a rig that is not empty;
 * MGF_ERR_CAPACITY: cap below mgf_batch_zone_count.  An empty rig: MGF_OK, nothing enqueued.  Synchronous: one download, one host wait. */
MGF_API mgf_status mgf_batch_read_zones_nearest(mgf_batch* b, int32_t k, int32_t* out, float* dist2_out, mgf_aabb* boxes_out, int64_t cap);
/* The same with the arrays in device memory (the device-pointer calls, above): enqueued on the context's stream and NOT waited for; in
 * the steady state no host wait and no copy between host and device.  Also refused with MGF_ERR_INVALID, nothing enqueued: a pointer
 * that fails the look-up of the device-pointer calls (4 (1 + k) count, 4 k count and 24 count bytes), and any two of the three arrays
 * overlapping. */
MGF_API mgf_status mgf_batch_read_zones_nearest_dev(mgf_batch* b, int32_t k, int32_t* out_dev, float* dist2_out_dev, mgf_aabb* boxes_out_dev, int64_t cap);
/* mgf_batch_overlap_first_dev with the nearest record, for boxes the caller computed on the device.  The fixed layout only: n must be a
 * multiple of n_worlds (else MGF_ERR_INVALID), box i is held against world i / (n / n_worlds); out_dev[(1 + k) * i ...] is the nearest
 * record of box i and dist2_out_dev[k * i ...] (NULL: not stored) its distances, with ignore_body_dev[i] (NULL: none) removed from its
 * list - only ever compared with a body index.  Refused with MGF_ERR_INVALID, nothing enqueued, in the order of
 * mgf_batch_overlap_first_dev: a NULL batch, a negative n or n > INT32_MAX, NULL boxes_dev / out_dev with n > 0, k outside
 * [0, MGF_BATCH_ZONE_NEAREST_MAX_K], n no multiple of n_worlds, a pointer that fails the look-up (boxes_dev 24 n bytes, ignore_body_dev
 * 4 n, out_dev 4 (1 + k) n, dist2_out_dev 4 k n), out_dev's or dist2_out_dev's bytes overlapping each other's or those of an input
 * array.  Not waited for; MGF_BATCH_NEAREST_LAUNCHES = 1 launch. */
MGF_API mgf_status mgf_batch_overlap_nearest_dev(mgf_batch* b, const mgf_aabb* boxes_dev, int64_t n, const int32_t* ignore_body_dev, int32_t k,
                                                 int32_t* out_dev, float* dist2_out_dev);
/* ---- contact sensors: touched by whom - the constraint list of the last tick folded per (body, partner), every word defined to the bit ----
 * mgf_batch_read_body_contacts sums over every partner of a body and separates the terrain only as a count.  "Is this foot on the ground,
 * and with what impulse", "did the agent reach that object", "is anything but the floor pushing on the torso", "where on the body is the
 * strongest contact" need the partner.  A contact sensor is the fourth rig of a batch beside ray sensors, cameras and zones: set once,
 * checked and sorted on the host, read every tick in one launch, a report of fixed width.  The struct and its definition are this
 * build's: the reference has no such report (its Solver keeps the list, solver.rs:53-79; nothing there folds it).  It reads no shapes,
 * so - unlike rays, sweeps, zones, sensors and cameras - it works on a batch that holds bodies of several components.
 * Sensor (world, body = x, other, flags).  L is the list mgf_batch_read_constraints(world) would return at that moment: the last tick's,
 * in insertion order; empty before the first tick and, for every world, once bodies have been added behind a tick; unchanged by
 * mgf_batch_write_state.
 * Chain: the records of L with a == x in ascending list index, then the records with b == x in ascending list index - the order
 * ContactConstraint::solve (solver.rs:203-252) meets them in, the order of mgf_body_contacts.
 * Partner of a chain record: b where x is `a` (-1 for RigidBodyRef::Static), a where x is `b`.
 * Match: other >= 0: the partner equals other; MGF_TOUCH_STATIC: the partner is -1 (terrain and obstacle contacts alike);
 * MGF_TOUCH_ANY_BODY: the partner is >= 0; MGF_TOUCH_ANY: always.
 * Fold over the matching records in chain order, impulse and normal_impulse starting at +0, ni = the record's normal_impulse and
 * t = (normal.x * ni, normal.y * ni, normal.z * ni):  x is `a`: impulse = impulse - t;  x is `b`: impulse = impulse + t;  in both roles
 * normal_impulse = normal_impulse + ni;  n_contacts counts the matching records.  Sequential f32 operations in that order, no fused
 * multiply-add.  So an MGF_TOUCH_ANY sensor's n_contacts, impulse and normal_impulse equal that body's mgf_body_contacts bit for bit, and
 * an MGF_TOUCH_STATIC sensor's n_contacts equals its n_terrain.
 * Strongest contact: the first matching record starts as the strongest; a later one replaces it only if its ni > the current one's, an
 * f32 compare - ties and NaN keep the earlier record.  Of that record: `record` is its list index within the world, `partner` its
 * partner, strongest_impulse its ni; push is its normal with every sign bit flipped where x is `a` and as stored where x is `b` - the
 * direction the impulse pushes x (solver.rs:243-247); arm is ra where x is `a` and rb where x is `b`.
 * Body frame: with MGF_TOUCH_BODY_FRAME and at least one match, impulse, push and arm are each replaced, after the fold, by
 * rotate((q.s, -q.x, -q.y, -q.z), v) with q the body's row as mgf_batch_read_state returns it at the moment of the read and rotate the
 * sensors' (tmp = q.v x v + v * q.s; (q.v x tmp) * 2 + v), every operation rounded on its own.  After mgf_batch_write_state the rotation
 * follows the new q AT ONCE; the list does not move.
 * No match, whatever the flags: n_contacts = 0, partner = MGF_TOUCH_NONE, record = -1, every other word +0.  reserved0 and reserved1
 * are always 0.  A report depends on its sensor and its world only: not on the other sensors, their order, or what else the batch holds.
 * A read writes nothing of the tick's state (not even `rows`, which mgf_batch_read_body_contacts rebuilds): a step after a read is
 * bit-identical to one without it.  mgf_batch_copy_worlds(_where) carries the list, so the destination's sensors answer as the
 * source's would.
 * "query_launches" of either read: MGF_BATCH_TOUCH_LAUNCHES = 1 whatever the worlds, sensors and list lengths; there is no collider
 * gather, since nothing here reads a shape.  No HIP events: "query_run_ns" is 0.
 * OUT OF SCOPE here: sums over the ticks of a multi-tick mgf_batch_step call (the report describes the last tick, as
 * mgf_batch_read_body_contacts does) (since: Rollout touch traces, below - mgf_batch_rollout_touches writes a report per tick, and a sum
 * is a reduction of its rows); tangent impulses (mgf_constraint does not carry them); groups of bodies as a partner filter; the k
 * strongest contacts rather than one; sensors on the lone mgf_world; a rig chosen per call by a device mask; hipGraph capture. */
#define MGF_TOUCH_STATIC   (-1)  /* RigidBodyRef::Static: the world's terrain and obstacles alike (b = -1) */
#define MGF_TOUCH_ANY_BODY (-2)  /* any body of the world */
#define MGF_TOUCH_ANY      (-3)  /* every record that names the body */
#define MGF_TOUCH_NONE     (-4)  /* mgf_touch_report.partner where nothing matched */
#define MGF_TOUCH_BODY_FRAME 1   /* flags: the three vectors in the frame of the body */
#define MGF_BATCH_TOUCH_LAUNCHES 1
typedef struct mgf_batch_touch { int32_t world, body, other, flags; } mgf_batch_touch;   /* 16 bytes */
typedef struct mgf_touch_report {
  int32_t n_contacts, partner, record, reserved0;
  mgf_vec3 impulse;  float normal_impulse;
  mgf_vec3 push;     float strongest_impulse;
  mgf_vec3 arm;      float reserved1;
} mgf_touch_report;                                                                       /* 64 bytes */
/* Replaces the rig; n = 0 clears it.  No device work: the rig goes up with the next read.  Refused with MGF_ERR_INVALID, the rig as it
 * was, in this order: what mgf_batch_set_sensors refuses - a NULL batch, a negative n or n > INT32_MAX, a NULL array with n > 0, then
 * per record a world out of range, a body outside [0, mgf_batch_len(b, world)) - then other < -3 or other >= mgf_batch_len(b, world),
 * other == body, a flag bit beyond MGF_TOUCH_BODY_FRAME.  The rig names (world, body): mgf_batch_add_bodies and
 * mgf_batch_add_compound_bodies afterwards leave every sensor on the bodies it named.  Independent of the other three rigs. */
MGF_API mgf_status mgf_batch_set_touches(mgf_batch* b, const mgf_batch_touch* t, int64_t n);
MGF_API int64_t    mgf_batch_touch_count(const mgf_batch* b);                 /* -1 for NULL */
/* The report of sensor i at out[i], in the order of the array given to mgf_batch_set_touches; cap: reports `out` holds.
 * MGF_ERR_INVALID: a NULL batch, a negative cap, NULL out with a rig that is not empty; MGF_ERR_CAPACITY: cap below
 * mgf_batch_touch_count, nothing written.  An empty rig: MGF_OK, nothing enqueued.  Synchronous: one launch, one download, one host wait. */
MGF_API mgf_status mgf_batch_read_touches(mgf_batch* b, mgf_touch_report* out, int64_t cap);
/* The same with the reports in device memory (the device-pointer calls, above): enqueued on the context's stream and NOT waited for; in
 * the steady state no host wait and no copy between host and device.  Also refused with MGF_ERR_INVALID, nothing enqueued: a pointer
 * that fails the look-up of the device-pointer calls (64 count bytes, aligned to 4 bytes). */
MGF_API mgf_status mgf_batch_read_touches_dev(mgf_batch* b, mgf_touch_report* out_dev, int64_t cap);
/* ---- body-mounted feelers: spheres and capsules with a displacement, fixed in the frame of a body, swept from the resident poses ----
 * A foothold or clearance probe ("can this foot come down here", "does my own body fit one step ahead"), the slope of the ground under
 * an agent, a bumper or whisker of finite thickness: the sweep is the one query whose answer carries a contact normal (mgf_ray_hit has
 * none), and a feeler is its rig - the fifth beside ray sensors, cameras, zones and contact sensors: set once, checked and sorted on the
 * host, cast every tick from the poses resident on the device.
 * A feeler is a record (world, body, tag, flags, p, d, r, delta): body an index within world; p, d and - without
 * MGF_FEELER_WORLD_DELTA - delta in the body's frame.  With x and q the body's rows as mgf_batch_read_state returns them - that is
 * x WITHOUT delta, the pose the sensors use - the feeler's cast C is
 *   shape: with MGF_FEELER_OWN_SHAPE, mgf_batch_read_colliders(world)[body].shape as it stands (tag, p, d, r of the record are not
 *          read); otherwise tag and r are the record's, P = x + rotate(q, p) and D = rotate(q, d) whatever the tag (a sphere's d is
 *          carried and not used, as by mgf_batch_sweep_many);
 *   displacement: with MGF_FEELER_WORLD_DELTA, C.delta = delta ("straight down" whatever the tilt); otherwise C.delta = rotate(q, delta);
 * rotate and the sum are the sensors' (Rotation::rotate_vector, a plain vector add, every operation a separate f32 one, no fused
 * multiply-add): C is defined to the bit.  The feeler's answer is, bit for bit, the mgf_sweep_hit that mgf_batch_sweep_many reports for
 * C against world `world` with the same kinds_mask and the ignore value `body` with MGF_FEELER_IGNORE_SELF, -1 without it.  Every rule
 * of that call holds unchanged, and nothing of the tick's state is touched.  On request the casts themselves come back as
 * mgf_moving_component, bit for bit the C above.
 * Poses written with mgf_batch_write_state, mgf_batch_set_many and the like move a feeler AT ONCE.  The colliders, and with them an
 * MGF_FEELER_OWN_SHAPE shape, move at the next tick.  (So behind a write an own-shape feeler casts the OLD collider along a delta turned
 * by the NEW q.)
 * A cast is MGF_BATCH_FEELER_LAUNCHES = 1 launch, one more where the mask asks for terrain and a world of the batch has a mesh, one more
 * where it asks for obstacles and a world has one, and the collider gather once behind a step ("query_launches") - whatever the number
 * of feelers and worlds; no plan, no index arrays.  No HIP events: "query_run_ns" is 0.
 * OUT OF SCOPE here: the parts of bodies of several components (LIMITS, above: both cast calls return MGF_ERR_INVALID,
 * "several components"; mgf_batch_set_feelers stays as it is); a kinds mask per feeler; more than one shape per record; feelers on the
 * lone mgf_world. */
#define MGF_FEELER_IGNORE_SELF 1   /* the body does not meet itself (the value of MGF_SENSOR_IGNORE_SELF) */
#define MGF_FEELER_WORLD_DELTA 2   /* delta is in world coordinates: "straight down" whatever the tilt */
#define MGF_FEELER_OWN_SHAPE   4   /* the cast is the body's own resident collider; tag, p, d, r are not read */
#define MGF_BATCH_FEELER_LAUNCHES 1  /* what one cast adds to "query_launches" without faces and obstacles */
typedef struct mgf_batch_feeler {
  int32_t world, body, tag, flags;
  mgf_vec3 p, d;
  float r;
  mgf_vec3 delta;
  int32_t reserved[2];     /* 0 */
} mgf_batch_feeler;        /* 64 bytes */
/* Replaces the rig by a copy of f[0 .. n); n = 0 clears it.  No device work: the rig goes up with the next cast.  Refused with
 * MGF_ERR_INVALID, the rig as it was ("the rig was not changed"), in this order: what mgf_batch_set_sensors refuses - a NULL batch, a
 * negative n or n > INT32_MAX, a NULL array with n > 0, then per record a world out of range, a body outside
 * [0, mgf_batch_len(b, world)) - then a flag bit beyond 7, a tag other than 0 or 1 without MGF_FEELER_OWN_SHAPE, MGF_FEELER_OWN_SHAPE
 * without MGF_FEELER_IGNORE_SELF (the body would meet itself at t = 0), a non-zero reserved word.  Radii, lengths and non-finite values
 * are not judged: mgf_batch_sweep_many does not judge them either, and the answer is defined as that call's.  The rig names
 * (world, body): mgf_batch_add_bodies and mgf_batch_add_compound_bodies afterwards leave every feeler on the body it named.
 * Independent of the other four rigs. */
MGF_API mgf_status mgf_batch_set_feelers(mgf_batch* b, const mgf_batch_feeler* f, int64_t n);
MGF_API int64_t    mgf_batch_feeler_count(const mgf_batch* b);                /* -1 for NULL */
/* The hit of feeler i at out[i], in the order of the array given to mgf_batch_set_feelers; casts_out non-NULL: also its cast C at
 * casts_out[i].  cap: records each array holds.  Refused in this order - MGF_ERR_INVALID: a NULL batch, a negative cap, a mask of 0 or
 * with bits beyond MGF_QUERY_ALL; MGF_ERR_CAPACITY: cap below mgf_batch_feeler_count; MGF_ERR_INVALID: NULL out with a rig that is not
 * empty, a batch that holds a body of several components.  An empty rig: MGF_OK, nothing enqueued.  Synchronous, as
 * mgf_batch_sweep_many: one download, one host wait. */
MGF_API mgf_status mgf_batch_cast_feelers(mgf_batch* b, int32_t kinds_mask, mgf_sweep_hit* out, mgf_moving_component* casts_out, int64_t cap);
/* The same with both arrays in device memory (the device-pointer calls, above): enqueued on the context's stream and NOT waited for.  In
 * the steady state no host wait and no copy between host and device.  Also refused with MGF_ERR_INVALID, nothing enqueued: a pointer
 * that fails the look-up of the device-pointer calls (52 * count bytes of out_dev, 44 * count of casts_out_dev), and out_dev's bytes
 * overlapping casts_out_dev's. */
MGF_API mgf_status mgf_batch_cast_feelers_dev(mgf_batch* b, int32_t kinds_mask, mgf_sweep_hit* out_dev, mgf_moving_component* casts_out_dev,
                                              int64_t cap);
/* ---- body-mounted actuators: directions and arms fixed in the frame of a body, wrenches formed from the resident poses ----
 * A rotor, a thruster, a wheel's drive, a reaction wheel, a foot pushing at its own point: the action-side mirror of the feeler, and
 * the sixth rig - set once, checked and sorted on the host, applied every tick from the poses resident on the device in one launch.
 * What a caller otherwise assembles per tick (mgf_batch_gather_state_dev for q, directions and arms turned in an expression of its own,
 * a cross product, a sum per body, mgf_batch_apply_impulses_dev) is here one call whose answer is defined to the bit.
 * An actuator is a record (world, body, flags, gain, p, lo, d, hi): body an index within world; the arm p in the body's frame; the
 * direction d in the body's frame or, with MGF_ACTUATOR_WORLD_DIR, the world's; one control value u[i] a call.
 * THE WRENCH of actuator i, with q the body's row as mgf_batch_read_state returns it at that moment - every line a separate f32
 * operation, no fused multiply-add:
 *   c = u[i];  if (c < lo) c = lo;  if (c > hi) c = hi;        (a NaN stays a NaN)
 *   s = gain * c
 *   e = WORLD_DIR ? d : rotate(q, d)                            rotate: the sensors' Rotation::rotate_vector
 *   TORQUE:      L = (0,0,0);  A = e * s
 *   otherwise:   L = e * s;  r = rotate(q, p);  A = cross(r, L)
 *                cross(a,b) = (a.y*b.z - a.z*b.y,  a.z*b.x - a.x*b.z,  a.x*b.y - a.y*b.x)
 *   s not finite: L = A = (0,0,0), and the actuator is counted in mgf_batch_counter "actuators_skipped"
 *                 (cumulative; reading it waits for the stream, like "device_skipped")
 * wrench_out is optional: when given it receives the six floats (L, A) of actuator i at row i, rows in the order of the array given
 * to mgf_batch_set_actuators.
 * WHAT A CALL DOES TO THE BATCH.  MGF_ACTUATE_IMPULSE: the batch ends bit for bit as after mgf_batch_apply_impulses(world, body, n,
 * L, A) with the rig's (world, body) and those wrenches in rig order - per body, in the caller's order, v = v + L * inv_mass,
 * omega = omega + I * A.  MGF_ACTUATE_FORCE: per body, in the caller's order, force = force + L, torque = torque + A - what
 * mgf_batch_get_many's force and torque rows, the same sequential f32 adds on the host and mgf_batch_set_forces give.  The force and
 * torque rows ACCUMULATE from call to call and hold for every later tick: a caller who wants "gravity plus this tick's thrust" writes
 * the rest rows first with mgf_batch_set_forces_dev, then calls this.  Nothing else of the tick's state is written: what
 * mgf_batch_set_forces and mgf_batch_apply_impulses leave alone stays alone, and a world no actuator names is untouched to the bit.
 * Actuators read no shapes: a batch with bodies of several components is answered, as by the contact sensors.
 * A pose written with mgf_batch_write_state, mgf_batch_set_many and the like turns the next wrench AT ONCE.
 * A call is MGF_BATCH_ACTUATOR_LAUNCHES = 1 launch, counted in "drive_launches", whatever the number of actuators and worlds: a lane
 * per body that has an actuator walks the body's actuators in the caller's order - no float atomic, nothing depends on lane scheduling.
 * OUT OF SCOPE here: actuators on the lone mgf_world; re-evaluation of a wrench per tick inside a multi-tick mgf_batch_step (a FORCE
 * wrench stays fixed in the world's frame until the next call) (since: Rollouts, below - mgf_batch_rollout); joints and motors between two bodies (spring-dampers since: Springs
 * between bodies, below - mgf_batch_set_springs; ball joints since: Ball joints between bodies, below - mgf_batch_set_joints; hinges
 * with limits and motors since: Hinge joints between bodies, below - mgf_batch_set_hinges). */
#define MGF_ACTUATOR_TORQUE     1   /* a pure couple about d: no force, p is not read */
#define MGF_ACTUATOR_WORLD_DIR  2   /* d is in world coordinates; the arm p stays in the body's frame */
#define MGF_ACTUATE_IMPULSE 0
#define MGF_ACTUATE_FORCE   1
#define MGF_BATCH_ACTUATOR_LAUNCHES 1  /* what one call adds to "drive_launches" */
typedef struct mgf_batch_actuator {
  int32_t world, body; uint32_t flags; float gain;
  mgf_vec3 p; float lo;
  mgf_vec3 d; float hi;
} mgf_batch_actuator;   /* 48 bytes: three 16-byte words */
/* Replaces the rig by a copy of a[0 .. n); n = 0 clears it.  No device work: the rig goes up with the next call.  Refused with
 * MGF_ERR_INVALID, the rig as it was ("the rig was not changed"), in this order: what mgf_batch_set_sensors refuses - a NULL batch, a
 * negative n or n > INT32_MAX, a NULL array with n > 0, then per record a world out of range, a body outside
 * [0, mgf_batch_len(b, world)) - then a flag bit beyond 3, a non-finite p, d or gain, a NaN lo or hi or lo > hi (-inf and +inf mean
 * "no clamp").  The rig names (world, body): mgf_batch_add_bodies and mgf_batch_add_compound_bodies afterwards leave every actuator on
 * the body it named.  Independent of the other five rigs. */
MGF_API mgf_status mgf_batch_set_actuators(mgf_batch* b, const mgf_batch_actuator* a, int64_t n);
MGF_API int64_t    mgf_batch_actuator_count(const mgf_batch* b);            /* -1 for NULL */
/* The wrenches of u[0 .. n) formed and applied (above).  Refused with MGF_ERR_INVALID in this order, nothing enqueued and nothing
 * changed: a NULL batch, a negative n, a mode other than MGF_ACTUATE_IMPULSE or MGF_ACTUATE_FORCE, n != mgf_batch_actuator_count(b) (a
 * control vector of the wrong length is a bug, not a prefix), NULL u with a rig that is not empty.  An empty rig: MGF_OK, nothing
 * enqueued.  Synchronous: one upload of u, one download where wrench_out is given, one host wait. */
MGF_API mgf_status mgf_batch_actuate(mgf_batch* b, const float* u, int64_t n, int32_t mode, float* wrench_out);
/* The same with both arrays in device memory (the device-pointer calls, above): enqueued on the context's stream and NOT waited for.  In
 * the steady state no host wait and no copy between host and device.  Also refused with MGF_ERR_INVALID, nothing enqueued: a pointer
 * that fails the look-up of the device-pointer calls (4 n bytes of u_dev, 24 n of wrench_out_dev), and wrench_out_dev's bytes
 * overlapping u_dev's. */
MGF_API mgf_status mgf_batch_actuate_dev(mgf_batch* b, const float* u_dev, int64_t n, int32_t mode, float* wrench_out_dev);
/* ---- rollouts: n_ticks ticks under n_ticks rows of controls, a row of state traced behind every tick, in ONE step call ----
 * The inner loop of sampling MPC, of trajectory optimisation and of any open-loop evaluation: a horizon of T ticks under T control
 * vectors, fanned out over the worlds of a batch (mgf_batch_copy_worlds copies one state to K worlds).  Call by call it costs T host
 * waits; a rollout is the same loop with the step's one.
 * THE DEFINITION is calls that exist, bit for bit.  With u[T][n_act], a mode, m flat body indices body[] (NULL: body i) and outputs
 * x[T][m][3], q[T][m][4], v[T][m][3], omega[T][m][3], any of them NULL, a rollout of T = n_ticks leaves the batch and the outputs as
 *   for t in 0 .. T-1:
 *     mgf_batch_actuate_dev(b, u[t], n_act, mode, NULL)                                        (skipped when n_act == 0)
 *     mgf_batch_step(b, dt, iters, 1, stats + t * n_worlds)
 *     mgf_batch_gather_state_dev(b, body, m, x[t], q[t], v[t], omega[t], NULL, NULL)           (skipped when m == 0)
 * leaves them: state, delta, the force and torque rows, the last tick's constraint lists, the stats rows, "actuators_skipped",
 * "device_skipped" (an index of body[] outside the batch is skipped and counted once a tick, its rows are not written), and what every
 * rig and reader reports afterwards - the last tick.  MGF_ACTUATE_FORCE accumulates from tick to tick exactly as the loop's calls
 * would.  n_act == 0 and nothing traced: mgf_batch_step(b, dt, iters, n_ticks, stats).  Actuators and the gather read no shapes: a batch
 * with bodies of several components is answered.
 * ONE HOST WAIT per pass of the step's re-run loop - one when no world outgrows its share of the storage.  A world whose tick did not
 * fit is undone, sits out the rest of the pass and is run again from that tick ("capacity_retries", as in the step); its control
 * row is applied ONCE all the same - the undo keeps tick t's impulse and never held the force rows, so the re-run does not actuate
 * again - and its trace rows are written in the pass in which it completes the tick.
 * The call adds at most MGF_BATCH_ROLLOUT_LAUNCHES_PER_TICK launches to a tick's own ("launches_per_tick" keeps its meaning and value):
 * one ahead of the tick where the rig is not empty, one behind it - whatever the worlds, the actuators and the traced bodies.
 * mgf_batch_counter "rollout_launches": the launches of the last rollout call beyond its ticks' own.  "drive_launches" is not touched.
 * REFUSED with MGF_ERR_INVALID, nothing enqueued and nothing changed, in this order - ahead of the handle's contents: a NULL batch; a
 * negative n_ticks, iters, n_act or m, in that order; n_ticks > 2^20; a mode other than MGF_ACTUATE_IMPULSE or MGF_ACTUATE_FORCE;
 * m > INT32_MAX; a byte count (4 * n_ticks * n_act; 16 * n_ticks * m cannot) that overflows int64_t - then the handle's own:
 * n_act != mgf_batch_actuator_count(b); NULL u with n_act > 0 and n_ticks > 0; body == NULL with m > mgf_batch_len(b, -1).
 * n_ticks == 0: MGF_OK, nothing enqueued beyond what mgf_batch_step(b, dt, iters, 0, stats) does.
 * OUT OF SCOPE here: closed-loop policies inside the call (u is fixed when the call is made); a step with no host wait at all; the
 * wrenches per tick; contact or touch sums per tick (the contact sensors' reports per tick since: Rollout touch traces, below -
 * mgf_batch_rollout_touches); a world mask; the lone mgf_world; hipGraph capture. */
#define MGF_BATCH_ROLLOUT_LAUNCHES_PER_TICK 2  /* what the call adds to a tick's launches, at most, with an empty spring rig */
/* The host form: one upload (u and body), the device core, one download (the outputs given).  stats: NULL or n_ticks * n_worlds rows,
 * row t * n_worlds + k world k's tick t.  A row of an index outside the batch comes back as zeros. */
MGF_API mgf_status mgf_batch_rollout(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u, int64_t n_act, int32_t mode,
                                     const int32_t* body, int64_t m, float* x, float* q, float* v, float* omega, mgf_step_stats* stats);
/* The same with u, body and the outputs in device memory (the device-pointer calls, above); stats stays host memory.  No copy between
 * host and device beyond the step's own.  Also refused with MGF_ERR_INVALID, nothing enqueued: a pointer that fails the look-up of the
 * device-pointer calls for its full extent (4 * n_ticks * n_act bytes of u_dev, 4 m of body_dev, 12 * n_ticks * m of x_dev, v_dev and
 * omega_dev, 16 * n_ticks * m of q_dev), an output's bytes overlapping another output's or an input's.  A row of an index outside the
 * batch is left as the caller had it. */
MGF_API mgf_status mgf_batch_rollout_dev(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u_dev, int64_t n_act, int32_t mode,
                                         const int32_t* body_dev, int64_t m, float* x_dev, float* q_dev, float* v_dev, float* omega_dev, mgf_step_stats* stats);
/* ---- springs between bodies: spring-dampers between two body-fixed points, impulses formed from the resident state ----
 * A tendon, a tether, a suspension strut, a soft hinge made of two springs, a body tied to a point of the world: the seventh rig and
 * the second on the action side - set once, checked and sorted on the host, applied from the state resident on the device.  What a
 * caller otherwise assembles per tick (mgf_batch_gather_state_dev of both ends, two arms turned by two quaternions, point velocities,
 * a length, a unit vector, a clamp, two cross products, a sum per body, mgf_batch_apply_impulses_dev) is here one call whose answer is
 * defined to the bit - and, ahead of every tick, part of a rollout.  No solver constraint: the reference has no joint (solver.rs knows
 * ContactConstraint only), and no tick kernel changes.
 * A spring is a record (world, body, other, flags, pa, rest, pb, k, c, lo, hi, pad): body and other indices within world; the arm pa
 * in body's frame; pb the arm in other's frame or, with other = -1, a point of the world; rest length, stiffness, damping and a clamp
 * [lo, hi] of the scalar force.  A rope is lo = 0, a strut that only pushes is hi = 0; -inf / +inf mean "no clamp".
 * THE WRENCH of spring i, with h the call's time step and x, q, v, omega of each end what mgf_batch_gather_state_dev returns at that
 * moment (x is x + delta) - every line a separate f32 operation, no fused multiply-add:
 *   ra = rotate(q_a, pa);  Pa = x_a + ra;  Va = v_a + cross(omega_a, ra)      rotate: the sensors' Rotation::rotate_vector, (q, vector)
 *   other >= 0:  rb = rotate(q_b, pb);  Pb = x_b + rb;  Vb = v_b + cross(omega_b, rb)
 *   other == -1: Pb = pb;  Vb = (0,0,0)
 *   d = Pb - Pa;  len = sqrt(dot(d, d));  n = d / len            (component-wise division)
 *                dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z;  cross(a,b) the actuators' (above), operands in the order written
 *   rate = dot(Vb - Va, n)
 *   f = k * (len - rest) + c * rate;  if (f < lo) f = lo;  if (f > hi) f = hi      (a NaN stays a NaN)
 *   s = f * h
 *   L = n * s;  A = cross(ra, L)                                  the impulse on `body`: pulled towards the far end for f > 0
 *   other >= 0:  Lb = -L;  Ab = cross(rb, Lb)                     the impulse on `other`
 *   len == 0, or len or s not finite:  all four vectors zero, and the spring is counted in mgf_batch_counter "springs_skipped"
 *                                      (cumulative; reading it waits for the stream, like "actuators_skipped")
 * wrench_out is optional: when given it receives the twelve floats (L, A, Lb, Ab) of spring i at row i - zeros for the far end of a
 * world anchor - rows in the order of the array given to mgf_batch_set_springs.
 * WHAT A CALL DOES TO THE BATCH.  Form the record list: for i in rig order (world_i, body_i, L, A), then, where other_i >= 0,
 * (world_i, other_i, Lb, Ab).  The batch ends, bit for bit, as after mgf_batch_apply_impulses of that list: per body, in list order,
 * v = v + L * inv_mass, omega = omega + I * A.  EVERY wrench is formed from the state before the call, whatever the order of the rig.
 * Nothing but velocities is written, and a world that no spring names is untouched to the bit.  Springs read no shapes: a batch with
 * bodies of several components is answered.
 * A call is at most MGF_BATCH_SPRING_LAUNCHES = 2 launches, counted in "drive_launches", whatever the number of springs and worlds: a
 * lane per spring forms the wrenches, then a lane per body that carries an end walks the body's ends in list order - no float atomic,
 * nothing depends on lane scheduling.
 * IN A ROLLOUT.  With a spring rig that is not empty, mgf_batch_rollout / _rollout_dev become, bit for bit, the loop
 *   mgf_batch_apply_springs_dev(b, dt, NULL) | mgf_batch_actuate_dev(u[t]) | mgf_batch_step(1) | mgf_batch_gather_state_dev(row t)
 * - the springs first, because a damper reads the velocities an impulse actuator writes.  Signatures, refusals and their order stay
 * as they are; with an empty spring rig the call is launch for launch what it was.  The springs add at most
 * MGF_BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK = 2 launches ahead of a tick, counted in "rollout_launches".  n_act == 0 with nothing
 * traced is then NOT mgf_batch_step: it is the stepping call of a batch with springs.  A world whose tick is undone and run again
 * gets tick t's springs ONCE, as it gets its control row once, and "springs_skipped" counts as the loop's calls would.
 * mgf_batch_step itself stays World::step, launch for launch: it applies no spring.
 * OUT OF SCOPE here: hard joints and limits in the solver (ball joints in a pass of their own since: Ball joints between bodies, below -
 * mgf_batch_set_joints; hinges with limits since: Hinge joints between bodies, below - mgf_batch_set_hinges); springs on the lone mgf_world; springs inside mgf_batch_step; the wrenches
 * per tick of a rollout; angular (torsion) springs; rest lengths or gains driven per tick from a control row. */
#define MGF_BATCH_SPRING_LAUNCHES 2  /* the most one call adds to "drive_launches" */
#define MGF_BATCH_ROLLOUT_SPRING_LAUNCHES_PER_TICK 2  /* what a spring rig that is not empty adds to a rollout's tick, at most */
typedef struct mgf_batch_spring {
  int32_t world, body, other; uint32_t flags;   /* other = -1: the far end is a point of the world; flags must be 0 */
  mgf_vec3 pa; float rest;                      /* arm in body's frame; rest length >= 0 */
  mgf_vec3 pb; float k;                         /* arm in other's frame, or the world point; stiffness */
  float c, lo, hi, pad;                         /* damping; clamp of the scalar force; pad = 0 */
} mgf_batch_spring;                             /* 64 bytes: four 16-byte words */
/* Replaces the rig by a copy of s[0 .. n); n = 0 clears it.  No device work: the rig goes up with the next call.  Refused with
 * MGF_ERR_INVALID, the rig as it was ("the rig was not changed"), in this order: what mgf_batch_set_sensors refuses - a NULL batch, a
 * negative n or n > INT32_MAX, a NULL array with n > 0, then per record a world out of range, a body outside
 * [0, mgf_batch_len(b, world)) - then other < -1 or other outside the world, other == body, flags != 0, a non-finite pa, pb, k, c or
 * rest, rest < 0, a NaN lo or hi or lo > hi.  The rig names (world, body) and (world, other): mgf_batch_add_bodies and
 * mgf_batch_add_compound_bodies afterwards leave every spring on the bodies it named.  Independent of the other six rigs. */
MGF_API mgf_status mgf_batch_set_springs(mgf_batch* b, const mgf_batch_spring* s, int64_t n);
MGF_API int64_t    mgf_batch_spring_count(const mgf_batch* b);              /* -1 for NULL */
/* The wrenches formed and applied (above).  Refused with MGF_ERR_INVALID, nothing enqueued and nothing changed: a NULL batch, a
 * non-finite h.  An empty rig: MGF_OK, nothing enqueued.  Synchronous: one download where wrench_out is given, one host wait. */
MGF_API mgf_status mgf_batch_apply_springs(mgf_batch* b, float h, float* wrench_out);
/* The same with wrench_out in device memory (the device-pointer calls, above): enqueued on the context's stream and NOT waited for.
 * Also refused with MGF_ERR_INVALID, nothing enqueued: a pointer that fails the look-up of the device-pointer calls (48 bytes a
 * spring of wrench_out_dev). */
MGF_API mgf_status mgf_batch_apply_springs_dev(mgf_batch* b, float h, float* wrench_out_dev);
/* ---- ball joints between bodies: point-to-point constraints, solved by sequential impulses from the resident state ----
 * A limb on a torso, a rope or a chain (a row of joints), a hinge (two joints on the hinge axis), a body pinned to the world (a joint
 * with a world anchor): the eighth rig and the spring's hard counterpart.  A spring is an explicit force - to hold two points together
 * it needs a stiffness the tick's time step cannot carry, and it lets them drift apart under load; a joint makes the VELOCITIES of its
 * two anchor points agree and removes a share of their gap per call.  The reference has no joint (solver.rs knows ContactConstraint
 * only), so this is the build's own definition, as the springs are; no tick kernel changes and mgf_batch_step applies no joint: the
 * joints are a pass of their own over the resident velocities, meant to run behind every external impulse and just ahead of the tick
 * that integrates them - which is where a rollout puts it (below).
 * A joint is a record (world, body, other, flags, pa, beta, pb, pad): body and other indices within world; pa the anchor in body's
 * frame; pb the anchor in other's frame or, with other = -1, a point of the world; beta in [0, 1] the share of the position error
 * removed per call (Baumgarte); flags and pad must be 0.
 * ONE CALL, mgf_batch_solve_joints(b, h, iters, impulse_out), reads of each end x (= x + delta) and q as
 * mgf_batch_gather_state_dev returns them, v and omega, and im and the 3x3 I - the inverse mass and the inverse inertia that
 * mgf_batch_apply_impulses uses.  Every line below is a separate rounded f32 operation, no fused multiply-add; rotate is the
 * sensors' Rotation::rotate_vector, (q, vector); dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z; cross(a,b) the actuators' (above), operands
 * in the order written; M * v row by row, (m.c[0].r * v.x + m.c[1].r * v.y) + m.c[2].r * v.z; invert is cgmath's SquareMatrix::invert:
 * det = c0.x * (c1.y * c2.z - c2.y * c1.z) - c1.x * (c0.y * c2.z - c2.y * c0.z) + c2.x * (c0.y * c1.z - c1.y * c0.z), the rows of the
 * inverse cross(c1, c2) / det, cross(c2, c0) / det, cross(c0, c1) / det.
 * SETUP, per joint i, from the state BEFORE the call:
 *   ra = rotate(q_a, pa);  Pa = x_a + ra
 *   other >= 0:  rb = rotate(q_b, pb);  Pb = x_b + rb;  im_b, I_b the body's
 *   other == -1: rb = 0;  Pb = pb;  im_b = 0;  I_b = 0
 *   C = Pb - Pa;  s = beta / h;  bias = C * s
 *   column k of K, e_k the unit vector:
 *       (e_k * im_a + cross(I_a * cross(ra, e_k), ra)) + (e_k * im_b + cross(I_b * cross(rb, e_k), rb))
 *   Kinv = invert(K)
 * A joint is SKIPPED if invert fails (det == 0) or any word of ra, rb, bias or Kinv is not finite: it is counted in
 * mgf_batch_counter "joints_skipped" (cumulative; reading it waits for the stream, like "springs_skipped"), touches no velocity and
 * reports a zero impulse - and it still takes its place in the order.
 * SWEEPS, iters times, over the joints of a world in the order of the array given to mgf_batch_set_joints; worlds are independent:
 *   Va = v_a + cross(omega_a, ra);  Vb = v_b + cross(omega_b, rb)      (other == -1: Vb = 0)
 *   P = Kinv * ((Vb - Va) + bias)
 *   v_a = v_a + P * im_a;  omega_a = omega_a + I_a * cross(ra, P)
 *   Pn = -P;  v_b = v_b + Pn * im_b;  omega_b = omega_b + I_b * cross(rb, Pn)   (other >= 0 only)
 *   acc_i = acc_i + P
 * Nothing but v and omega is written; a body that no joint names is untouched to the bit, and so is a world that no joint names.
 * impulse_out is optional: when given, row i receives acc_i, three floats - the joint's reaction over the call - rows in the order
 * of the array given to mgf_batch_set_joints.  There is no warm start: no state is kept between calls.  Joints read no shapes: a batch
 * with bodies of several components is answered.
 * A call is MGF_BATCH_JOINT_LAUNCHES = 1 launch, counted in "drive_launches", whatever the number of joints and worlds: a workgroup
 * per world that has joints, a lane per joint - hence at most MGF_BATCH_MAX_WORLD_JOINTS = 256 joints a world - which solves its
 * joint as soon as both its bodies have been through the joints listed ahead of it; no float atomic, and the result does not depend
 * on lane scheduling.
 * IN A ROLLOUT.  With a joint rig that is not empty, mgf_batch_rollout and its _dev, _touches and _observe forms become, bit for bit,
 * the loop
 *   [mgf_batch_apply_springs_dev(dt)] | mgf_batch_actuate_dev(u[t]) | mgf_batch_solve_joints_dev(b, dt, iters, NULL) | mgf_batch_step(dt, iters, 1) |
 *   mgf_batch_gather_state_dev(row t) | [traces]
 * - the joints behind every external impulse, with the call's own iters: there is no new argument and no new option.  Signatures,
 * refusals and their order stay as they are; with an empty joint rig every call is launch for launch what it was.  The joints add
 * MGF_BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK = 1 launch to a tick, counted in "rollout_launches".  n_act == 0 with nothing traced is
 * then NOT mgf_batch_step: it is the stepping call of a batch with joints.  A world whose tick is undone and run again gets tick t's
 * joints ONCE, as it gets its springs once, and "joints_skipped" counts as the loop's calls would.
 * mgf_batch_step itself stays World::step, launch for launch: it applies no joint.
 * OUT OF SCOPE here: joints inside the tick's solver, coupled with the contacts in one sweep; angular rows, limits and motors (a
 * hinge is two joints); warm starting; more than MGF_BATCH_MAX_WORLD_JOINTS joints a world; joints on the lone mgf_world;
 * joints inside mgf_batch_step; the impulses per tick of a rollout; beta or anchors driven per tick from a control row.
 * (Angular rows, limits and motors since: Hinge joints between bodies, below - mgf_batch_set_hinges, whose motors are driven per tick
 * from a table.) */
#define MGF_BATCH_JOINT_LAUNCHES 1  /* what one solve call adds to "drive_launches" */
#define MGF_BATCH_ROLLOUT_JOINT_LAUNCHES_PER_TICK 1  /* what a joint rig that is not empty adds to a rollout's tick */
#define MGF_BATCH_MAX_WORLD_JOINTS 256  /* joints one world holds at most */
typedef struct mgf_batch_joint {
  int32_t world, body, other; uint32_t flags;   /* other = -1: the far end is a point of the world; flags must be 0 */
  mgf_vec3 pa; float beta;                      /* anchor in body's frame; the share of the position error removed per call, in [0, 1] */
  mgf_vec3 pb; float pad;                       /* anchor in other's frame, or the world point; pad = 0 */
} mgf_batch_joint;                              /* 48 bytes: three 16-byte words */
/* Replaces the rig by a copy of j[0 .. n); n = 0 clears it.  No device work: the rig goes up with the next call.  Refused with
 * MGF_ERR_INVALID, the rig as it was ("the rig was not changed"), in this order: what mgf_batch_set_sensors refuses - a NULL batch, a
 * negative n or n > INT32_MAX, a NULL array with n > 0, then per record a world out of range, a body outside
 * [0, mgf_batch_len(b, world)) - then other < -1 or other outside the world, other == body, flags != 0 or pad != 0, a non-finite pa
 * or pb, a beta that is not finite or outside [0, 1], a world's joint beyond its MGF_BATCH_MAX_WORLD_JOINTS-th.  The rig names
 * (world, body) and (world, other): mgf_batch_add_bodies and mgf_batch_add_compound_bodies afterwards leave every joint on the bodies
 * it named.  Independent of the other seven rigs. */
MGF_API mgf_status mgf_batch_set_joints(mgf_batch* b, const mgf_batch_joint* j, int64_t n);
MGF_API int64_t    mgf_batch_joint_count(const mgf_batch* b);               /* -1 for NULL */
/* The joints solved (above).  Refused with MGF_ERR_INVALID, nothing enqueued and nothing changed, in this order: a NULL batch, a
 * non-finite h, iters < 0.  iters == 0 or an empty rig: MGF_OK, nothing enqueued, impulse_out not written.  Synchronous: one download
 * where impulse_out is given, one host wait.  MGF_ERR_HIP "internal error" behind the wait: a lane gave up waiting for its turn - a
 * bug, never a wait for another workgroup; the world's velocities are then as the call found them. */
MGF_API mgf_status mgf_batch_solve_joints(mgf_batch* b, float h, int32_t iters, float* impulse_out);
/* The same with impulse_out in device memory (the device-pointer calls, above): enqueued on the context's stream and NOT waited for.
 * Also refused with MGF_ERR_INVALID, nothing enqueued: a pointer that fails the look-up of the device-pointer calls (12 bytes a
 * joint of impulse_out_dev). */
MGF_API mgf_status mgf_batch_solve_joints_dev(mgf_batch* b, float h, int32_t iters, float* impulse_out_dev);
/* ---- hinge joints between bodies: a point, two angular rows, a limit and a motor, solved from the resident state ----
 * A knee, an elbow, a gripper's finger, a wheel on an axle, a door: a revolute joint with a range and a drive - the ninth rig.  A ball
 * joint (above) leaves all three rotations free, and two of them on an axis give the axis and nothing more: no limit, so a knee folds
 * through itself, and no motor, so a policy can only throw external wrenches that do not react on the other body.  A hinge is
 *   - a point constraint, solved as the ball joint's;
 *   - two angular rows that keep the hinge axis of `body` and that of `other` parallel;
 *   - with MGF_HINGE_LIMIT a limit lo <= theta <= hi of the hinge angle;
 *   - with MGF_HINGE_MOTOR a velocity motor: the relative speed about the axis driven to a target, the torque capped at tmax; the
 *     target comes from a table of the handle's, a row a call (a rollout: a row a tick), so that a policy can drive it.
 * The reference has no joint, so this is the build's own definition, as the ball joints are; no tick kernel changes and
 * mgf_batch_step applies no hinge: the hinges are a pass of their own over the resident velocities.
 * A hinge is a record (world, body, other, flags, pa, beta, pb, tmax, ax, cm, ua, sm, bx, ch, ub, sh): body and other indices within
 * world (other = -1: the far end is the world); pa, ax, ua the anchor, the unit hinge axis and a unit zero-angle reference
 * perpendicular to it in body's frame; pb, bx, ub the same in other's frame, or the world's; beta in [0, 1] the share of the
 * position error removed per call, used by the point, angular and limit rows; tmax >= 0 the motor's largest torque (+inf allowed);
 * (cm, sm) = (cos, sin) of mid = (lo + hi) / 2 and (ch, sh) = (cos, sin) of half = (hi - lo) / 2 in [0, pi], so sh >= 0.  With
 * A, T1, T2 the axis, the reference and their cross product of `body` in the world and U1 the reference of `other` there (below), the
 * hinge angle is theta = atan2(dot(U1, T2), dot(U1, T1)) - the angle of other's reference about body's axis - and its rate is
 * dot(omega_b - omega_a, A).  NO arctangent is ever evaluated: the limit is held through the four cosines and sines of the record, so
 * the definition uses + - * / and comparisons alone.
 * ONE CALL, mgf_batch_solve_hinges(b, h, iters, row, impulse_out), reads what mgf_batch_solve_joints reads of each end.  Every line
 * below is a separate rounded f32 operation, no fused multiply-add; rotate, cross, dot, M * v and invert are the ball joints' (above);
 * a sum or product of three terms is taken left to right; -x / y is (-x) / y.
 * SETUP, per hinge i, from the state BEFORE the call:
 *   ra, rb, Pa, Pb, C, s = beta / h, bias, K, Kinv: the ball joint's lines, with this record's pa, pb and beta
 *   A = rotate(q_a, ax);  T1 = rotate(q_a, ua);  T2 = cross(A, T1)
 *   other >= 0:  B = rotate(q_b, bx);  U1 = rotate(q_b, ub)
 *   other == -1: B = bx;  U1 = ub;  omega_b = 0;  I_b = 0
 *   n1 = cross(B, T1);  n2 = cross(B, T2);  g1 = dot(B, T1) * s;  g2 = dot(B, T2) * s
 *   J(n) = I_a * n + I_b * n
 *   k11 = dot(n1, J(n1));  k12 = dot(n1, J(n2));  k21 = dot(n2, J(n1));  k22 = dot(n2, J(n2));  d2 = k11 * k22 - k12 * k21
 *   m11 = k22 / d2;  m12 = -k12 / d2;  m21 = -k21 / d2;  m22 = k11 / d2
 *   Km = dot(A, J(A))
 *   c = dot(U1, T1);  sn = dot(U1, T2);  cphi = c * cm + sn * sm;  sphi = sn * cm - c * sm
 *   LIMIT and cphi <= ch:  err = fabs(sphi) * ch - cphi * sh;  sphi >= 0: side = +1, lb = -(err * s);  else side = -1, lb = err * s
 *   otherwise side = 0, lb = 0    (the limit row is off for this call: a limit acts from the call after the angle passed it)
 *   MOTOR:  mmax = tmax * h;  w = entry i of the target table's row for this call (below)
 * A hinge is SKIPPED on any of: what skips a ball joint (det == 0, a word of ra, rb, bias or Kinv not finite); d2 == 0; Km == 0 with
 * either flag set; a word of n1, n2, g1, g2, m11, m12, m21, m22, Km or lb not finite; with MOTOR a NaN mmax or a w that is not finite.
 * It is counted in mgf_batch_counter "hinges_skipped" (cumulative; reading it waits for the stream), touches no velocity and reports
 * zeros - and it still takes its place in the order.
 * SWEEPS, iters times, over the hinges of a world in the order of the array given to mgf_batch_set_hinges; worlds are independent.
 * The rows of one hinge in this order, wd = omega_b - omega_a formed again from the current velocities ahead of each of the first
 * three (other == -1: omega_b is the zero vector and is not written), am, al, a1, a2, acc starting from 0 with the call:
 *   MOTOR:    lam = (w - dot(wd, A)) / Km;  t = am + lam;  if (t < -mmax) t = -mmax;  if (t > mmax) t = mmax;  lam = t - am;  am = t
 *             imp = A * lam;  omega_a = omega_a - I_a * imp;  omega_b = omega_b + I_b * imp
 *   side!=0:  lam = (lb - dot(wd, A)) / Km;  t = al + lam;  side < 0: if (t < 0) t = 0;  side > 0: if (t > 0) t = 0;  lam = t - al;  al = t
 *             imp = A * lam;  the same two updates
 *   angular:  r1 = dot(wd, n1) + g1;  r2 = dot(wd, n2) + g2;  l1 = -(m11 * r1 + m12 * r2);  l2 = -(m21 * r1 + m22 * r2)
 *             imp = n1 * l1 + n2 * l2;  the same two updates;  a1 = a1 + l1;  a2 = a2 + l2
 *   point:    Va = v_a + cross(omega_a, ra);  Vb = v_b + cross(omega_b, rb)  (other == -1: Vb = 0);  P = Kinv * ((Vb - Va) + bias)
 *             v_a = v_a + P * im_a;  omega_a = omega_a + I_a * cross(ra, P)
 *             Pn = -P;  v_b = v_b + Pn * im_b;  omega_b = omega_b + I_b * cross(rb, Pn)   (other >= 0 only);  acc = acc + P
 * Nothing but v and omega is written; a body that no hinge names is untouched to the bit, and so is a world that no hinge names.
 * impulse_out is optional: when given, row i receives eight floats, (acc.x, acc.y, acc.z, a1, a2, al, am, 0) - the point's reaction,
 * the two angular impulses, the limit's and the motor's over the call.  There is no warm start: no state is kept between calls.
 * Hinges read no shapes: a batch with bodies of several components is answered.
 * THE TARGET TABLE.  The handle owns W[rows][mgf_batch_hinge_count] floats in device memory: mgf_batch_set_hinge_targets copies it
 * from host memory, mgf_batch_set_hinge_targets_dev from device memory; a solve call names the row it reads.  Only hinges with MOTOR
 * read their column.  A motor with target 0 is a brake; one with tmax = +inf and target 0 locks the angle's rate.
 * mgf_batch_set_hinges makes the table one row of zeros.
 * A call is MGF_BATCH_HINGE_LAUNCHES = 1 launch, counted in "drive_launches", whatever the number of hinges and worlds: a workgroup
 * per world that has hinges, a lane per hinge - hence at most MGF_BATCH_MAX_WORLD_HINGES = 256 hinges a world - which solves all four
 * rows of its hinge as soon as both its bodies have been through the hinges listed ahead of it; no float atomic, and the result does
 * not depend on lane scheduling.
 * IN A ROLLOUT.  With a hinge rig that is not empty, mgf_batch_rollout and its _dev, _touches and _observe forms become, bit for bit,
 * the loop
 *   [mgf_batch_apply_springs_dev(dt)] | mgf_batch_actuate_dev(u[t]) | [mgf_batch_solve_joints_dev(b, dt, iters, NULL)] |
 *   mgf_batch_solve_hinges_dev(b, dt, iters, min(t, rows - 1), NULL) | mgf_batch_step(dt, iters, 1) | mgf_batch_gather_state_dev(row t) | [traces]
 * - a table of one row holds its targets for the whole call, a table of T rows is a control tape, a row a tick.  Signatures, refusals
 * and their order stay as they are; with an empty hinge rig every call is launch for launch what it was.  The hinges add
 * MGF_BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK = 1 launch to a tick, counted in "rollout_launches".  n_act == 0 with nothing traced is
 * then NOT mgf_batch_step.  A world whose tick is undone and run again gets tick t's hinges ONCE, and "hinges_skipped" counts as the
 * loop's calls would.  mgf_batch_step itself stays World::step, launch for launch: it applies no hinge.
 * OUT OF SCOPE here: hinges and ball joints in one interleaved sweep, or inside the tick's solver with the contacts; position (servo)
 * motors, joint friction beyond a zero-target motor, prismatic and fixed joints; warm starting; limits that act speculatively before
 * the angle passes them; more than MGF_BATCH_MAX_WORLD_HINGES hinges a world; hinges on the lone mgf_world;
 * hinges inside mgf_batch_step; the impulses per tick of a rollout; joint angle and rate as a traced observation.
 * (The impulses per tick, and angle and rate as a call and as a traced observation since: Hinge encoders, below -
 * mgf_batch_read_hinges, mgf_batch_set_hinge_trace.  Prismatic and fixed joints since: Sliders between bodies, below -
 * mgf_batch_set_sliders.) */
#define MGF_HINGE_LIMIT 1  /* the hinge angle is held to [lo, hi] through cm, sm, ch, sh */
#define MGF_HINGE_MOTOR 2  /* the relative speed about the axis is driven to the table's target, the torque capped at tmax */
#define MGF_BATCH_HINGE_LAUNCHES 1  /* what one solve call adds to "drive_launches" */
#define MGF_BATCH_ROLLOUT_HINGE_LAUNCHES_PER_TICK 1  /* what a hinge rig that is not empty adds to a rollout's tick */
#define MGF_BATCH_MAX_WORLD_HINGES 256  /* hinges one world holds at most */
typedef struct mgf_batch_hinge {
  int32_t world, body, other; uint32_t flags;   /* other = -1: the far end is the world; flags: MGF_HINGE_LIMIT | MGF_HINGE_MOTOR */
  mgf_vec3 pa; float beta;                      /* anchor in body's frame; Baumgarte share in [0, 1], used by the point, angular and limit rows */
  mgf_vec3 pb; float tmax;                      /* anchor in other's frame, or the world point; the motor's largest torque, >= 0, +inf allowed */
  mgf_vec3 ax; float cm;                        /* hinge axis in body's frame (unit); cos(mid), mid = (lo + hi) / 2 */
  mgf_vec3 ua; float sm;                        /* zero-angle reference in body's frame, unit, perpendicular to ax; sin(mid) */
  mgf_vec3 bx; float ch;                        /* hinge axis in other's frame, or the world's; cos(half), half = (hi - lo) / 2 in [0, pi] */
  mgf_vec3 ub; float sh;                        /* reference in other's frame, or the world's, unit, perpendicular to bx; sin(half) >= 0 */
} mgf_batch_hinge;                              /* 112 bytes: seven 16-byte words */
/* Replaces the rig by a copy of j[0 .. n); n = 0 clears it; the target table becomes one row of zeros.  No device work: the rig goes
 * up with the next call.  Refused with MGF_ERR_INVALID, the rig as it was ("the rig was not changed"), in this order: what
 * mgf_batch_set_joints refuses up to other == body, in its order; a flag bit beyond MGF_HINGE_LIMIT | MGF_HINGE_MOTOR; a word of the
 * record that is not finite (tmax may be +inf); beta outside [0, 1]; tmax < 0; then, in double on the host, |ax|^2, |ua|^2, |bx|^2,
 * |ub|^2, cm^2 + sm^2 or ch^2 + sh^2 more than 1e-3 away from 1; |dot(ax, ua)| or |dot(bx, ub)| above 1e-3; sh < 0; last a world's
 * hinge beyond its MGF_BATCH_MAX_WORLD_HINGES-th.  The rig names (world, body) and (world, other): mgf_batch_add_bodies and
 * mgf_batch_add_compound_bodies afterwards leave every hinge on the bodies it named.  Independent of the other eight rigs. */
MGF_API mgf_status mgf_batch_set_hinges(mgf_batch* b, const mgf_batch_hinge* j, int64_t n);
MGF_API int64_t    mgf_batch_hinge_count(const mgf_batch* b);               /* -1 for NULL */
/* The target table replaced by a copy of w[rows][mgf_batch_hinge_count] (host memory; one upload, waited for).  Refused with
 * MGF_ERR_INVALID, the table as it was, in this order: a NULL batch; rows < 1 or rows > 2^20; a NULL w with a rig that is not empty; a
 * byte count that overflows.  With an empty rig the number of rows is all that is kept. */
MGF_API mgf_status mgf_batch_set_hinge_targets(mgf_batch* b, const float* w, int64_t rows);
/* The same from device memory (the device-pointer calls, above): a device-to-device copy enqueued on the context's stream and NOT
 * waited for - w_dev may be written again once the stream has passed the copy.  Also refused, nothing enqueued: a pointer that fails
 * the look-up of the device-pointer calls (4 * rows * mgf_batch_hinge_count bytes of w_dev). */
MGF_API mgf_status mgf_batch_set_hinge_targets_dev(mgf_batch* b, const float* w_dev, int64_t rows);
/* The hinges solved (above), the motors' targets from row `row` of the table.  Refused with MGF_ERR_INVALID, nothing enqueued and
 * nothing changed, in this order: a NULL batch, a non-finite h, iters < 0, row outside [0, rows).  iters == 0 or an empty rig: MGF_OK,
 * nothing enqueued, impulse_out not written.  Synchronous: one download where impulse_out is given (32 bytes a hinge), one host wait.
 * MGF_ERR_HIP "internal error" behind the wait: a lane gave up waiting for its turn - a bug, never a wait for another workgroup; the
 * world's velocities are then as the call found them. */
MGF_API mgf_status mgf_batch_solve_hinges(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out);
/* The same with impulse_out in device memory (the device-pointer calls, above): enqueued on the context's stream and NOT waited for.
 * Also refused with MGF_ERR_INVALID, nothing enqueued: a pointer that fails the look-up of the device-pointer calls (32 bytes a
 * hinge of impulse_out_dev). */
MGF_API mgf_status mgf_batch_solve_hinges_dev(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out_dev);
/* ---- hinge encoders: angle, rate, limit side, gap and tilt of every hinge, read from the resident state and traced per tick ----
 * A policy that drives a knee has to feel it: the hinge angle and its rate are the first two numbers a controller reads of a joint, a
 * planner's cost wants them - and the torque the motor spent - at every tick of the horizon, and whoever tunes beta and iters wants to
 * know how far the anchors gap and the axes tilt under load.  A READING is eight floats, 32 bytes,
 *   (c, sn, rate, side, gap.x, gap.y, gap.z, tilt2)
 * formed from the state AS IT STANDS by the SETUP lines of the hinge section above, verbatim, with the same helpers (rotate, cross,
 * dot); every line below is a separate rounded f32 operation, no fused multiply-add:
 *   ra, rb, Pa, Pb, C, A, T1, T2, B, U1: SETUP's lines (other == -1: B = bx, U1 = ub, Pb = pb, omega_b = 0)
 *   c = dot(U1, T1);  sn = dot(U1, T2)         the hinge angle is theta = atan2(sn, c); NO arctangent is evaluated on the device
 *   rate = dot(omega_b - omega_a, A)
 *   cphi = c * cm + sn * sm;  sphi = sn * cm - c * sm
 *   LIMIT and cphi <= ch:  sphi >= 0: side = +1.0f;  else side = -1.0f;  otherwise side = 0.0f
 *                                              - whether the NEXT solve's limit row would be on, and on which side
 *   gap = C                                    the anchors' gap in the world
 *   e1 = dot(B, T1);  e2 = dot(B, T2);  tilt2 = e1 * e1 + e2 * e2      the squared sine of the angle between the two axes
 * There is no division: no hinge is skipped and there is no counter.  Non-finite state gives non-finite words.  A reading reads no
 * shapes - a batch with bodies of several components is answered - and writes nothing but its output: the state is untouched to the bit.
 * ONE CALL, mgf_batch_read_hinges(b, out), is MGF_BATCH_HINGE_READ_LAUNCHES = 1 launch, counted in "drive_launches" as the solve's is: a
 * lane per hinge by the caller's index over all worlds.  What set_many, mgf_batch_add_bodies or mgf_batch_set_hinges left on the host
 * goes up first, by the path the solve uses.
 * THE READINGS TABLE.  mgf_rollout_traces has no word left for it, so the trace mirrors the target table: targets are a table in, a
 * row a tick; readings are a table out, a row a tick.  mgf_batch_set_hinge_trace(b, rows, format) makes the handle allocate and zero
 * R[rows][mgf_batch_hinge_count] entries in device memory; rows == 0 frees it and turns the trace off, which is the default, and
 * mgf_batch_set_hinges sets it back to 0 rows as it resets the target table.  An entry is
 *   MGF_HINGE_TRACE_READING  32 bytes: the reading;
 *   MGF_HINGE_TRACE_FULL     64 bytes: the reading, then the eight floats (acc.x, acc.y, acc.z, a1, a2, al, am, 0) of tick t's hinge
 *                            solve - am / dt is the torque the motor applied in tick t, al / dt the limit's.
 * IN A ROLLOUT.  With a hinge rig that is not empty and rows > 0, mgf_batch_rollout and its _dev, _touches, _touches_dev, _observe and
 * _observe_dev forms - no new entry point, no changed signature - are the defining loop of the hinge section with one more line at the
 * end of tick t < rows:
 *   ... | mgf_batch_step(dt, iters, 1) | mgf_batch_gather_state_dev(row t) | [traces] | mgf_batch_read_hinges_dev(b, row t)
 * and every row is bit for bit what that loop gives; for FULL the impulse words are those of tick t's
 * mgf_batch_solve_hinges_dev(..., impulse_out) in that loop, and zeros with iters == 0, where no solve is enqueued.  Ticks t >= rows
 * write nothing and launch nothing - there is NO clamp: an output is never overwritten silently - and rows the call does not reach stay
 * as they were.  The trace adds MGF_BATCH_ROLLOUT_HINGE_READ_LAUNCHES_PER_TICK = 1 launch to a tick that has a row, behind the state
 * trace's, counted in "rollout_launches"; with rows == 0 or an empty rig every rollout is launch for launch what it was.  A world
 * whose tick is undone and run again gets its row t in the pass in which it completes t, with the impulses of the pass that solved t.
 * OUT OF SCOPE here: position (servo) motors; readings for ball joints; readings inside mgf_rollout_traces; a clamp or ring-buffer
 * mode of the table; the lone mgf_world; hipGraph capture. */
#define MGF_BATCH_HINGE_READ_LAUNCHES 1  /* what one read call adds to "drive_launches" */
#define MGF_BATCH_ROLLOUT_HINGE_READ_LAUNCHES_PER_TICK 1  /* what the readings table adds to a rollout's tick t < rows */
#define MGF_HINGE_TRACE_READING 0  /* an entry of the table is the 32-byte reading */
#define MGF_HINGE_TRACE_FULL 1     /* 64 bytes: the reading and the eight impulse words of the tick's hinge solve */
typedef struct mgf_hinge_reading {
  float c, sn;     /* cosine and sine of the hinge angle: theta = atan2(sn, c) */
  float rate;      /* dot(omega_b - omega_a, A), rad/s */
  float side;      /* +1 or -1: LIMIT is set and the angle is past hi or lo - the next solve's limit row is on; 0: it is off */
  mgf_vec3 gap;    /* Pb - Pa, the anchors' gap in the world */
  float tilt2;     /* the squared sine of the angle between the two hinge axes */
} mgf_hinge_reading;  /* 32 bytes: two 16-byte words */
/* The readings of every hinge into out[0 .. mgf_batch_hinge_count) (host memory): one download, one host wait.  Refused with
 * MGF_ERR_INVALID, nothing enqueued, in this order: a NULL batch; a NULL out with a rig that is not empty.  An empty rig: MGF_OK,
 * nothing enqueued. */
MGF_API mgf_status mgf_batch_read_hinges(mgf_batch* b, mgf_hinge_reading* out);
/* The same with out in device memory (the device-pointer calls, above): enqueued on the context's stream and NOT waited for.  Also
 * refused with MGF_ERR_INVALID, nothing enqueued: a pointer that fails the look-up of the device-pointer calls (32 bytes a hinge of
 * out_dev), or that is not aligned to 16 bytes - the readings are stored as 16-byte words. */
MGF_API mgf_status mgf_batch_read_hinges_dev(mgf_batch* b, mgf_hinge_reading* out_dev);
/* The readings table made rows x mgf_batch_hinge_count entries of zeros in `format`; rows == 0: freed, no trace.  Refused with
 * MGF_ERR_INVALID, the table as it was, in this order: a NULL batch; rows < 0 or rows > 2^20; a format that is neither
 * MGF_HINGE_TRACE_READING nor MGF_HINGE_TRACE_FULL; a byte count that overflows.  With an empty rig rows and format are all that is kept. */
MGF_API mgf_status mgf_batch_set_hinge_trace(mgf_batch* b, int64_t rows, int32_t format);
MGF_API int64_t    mgf_batch_hinge_trace_rows(const mgf_batch* b);          /* -1 for NULL */
/* Rows [row0, row0 + n_rows) of the table into out (host memory, n_rows x mgf_batch_hinge_count entries of 32 or 64 bytes): one
 * download, waited for.  Refused with MGF_ERR_INVALID, in this order: a NULL batch; row0 < 0; n_rows < 0; row0 + n_rows beyond the
 * table's rows; a NULL out with bytes to copy. */
MGF_API mgf_status mgf_batch_get_hinge_trace(mgf_batch* b, void* out, int64_t row0, int64_t n_rows);
/* The same as a device-to-device copy, enqueued on the context's stream and NOT waited for.  Also refused, nothing enqueued: a pointer
 * that fails the look-up of the device-pointer calls. */
MGF_API mgf_status mgf_batch_get_hinge_trace_dev(mgf_batch* b, void* out_dev, int64_t row0, int64_t n_rows);
/* ---- rollout touch traces: the contact sensors' reports behind every tick of a rollout ----
 * A rollout records the STATE of chosen bodies behind every tick.  A sampling planner or a cost function also asks "did the foot
 * touch, how hard, and what touched it" at every tick of the horizon; call by call that is T host waits again.  These two calls are
 * mgf_batch_rollout / _rollout_dev with one more output: row t of the reports of the contact sensors' rig (mgf_batch_set_touches)
 * behind tick t.
 * THE DEFINITION is calls that exist, bit for bit.  With touch[T][n_touch] in the rig's order, the batch and every output are left as
 *   for t in 0 .. T-1:
 *     mgf_batch_apply_springs_dev(b, dt, NULL)                                                  (with a spring rig that is not empty)
 *     mgf_batch_actuate_dev(b, u[t], n_act, mode, NULL)                                        (skipped when n_act == 0)
 *     mgf_batch_step(b, dt, iters, 1, stats + t * n_worlds)
 *     mgf_batch_gather_state_dev(b, body, m, x[t], q[t], v[t], omega[t], NULL, NULL)           (skipped when m == 0)
 *     mgf_batch_read_touches_dev(b, touch + t * n_touch, n_touch)
 * leaves them.  touch_format MGF_ROLLOUT_TOUCH_FULL: an entry is that mgf_touch_report, 64 bytes.  MGF_ROLLOUT_TOUCH_SHORT: an entry
 * is 16 bytes - the words n_contacts, partner, normal_impulse, strongest_impulse of that report, in this order - for a caller who
 * asks "touched, by whom, how hard" and wants a quarter of the traffic.  EVERY entry is written: every world completes every tick of
 * a call that returns MGF_OK.  MGF_TOUCH_BODY_FRAME turns the vectors by the body's q behind tick t, as a read between the ticks
 * does.  The reports read no shapes: a batch with bodies of several components is answered, as by both parents.
 * touch == NULL, or n_touch == 0 with an empty rig: the call IS mgf_batch_rollout / _rollout_dev, launch for launch.
 * ONE HOST WAIT per pass, as in a rollout.  A world whose tick t did not fit is undone and skipped by this launch as by every other of
 * the pass; its row t is written in the pass in which it completes t, and never from a list that a later, undone tick wrote into.
 * The trace adds MGF_BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK = 1 launch behind a tick in every pass that runs it, whatever the worlds,
 * the sensors and the list lengths, counted in "rollout_launches"; "query_launches" and "drive_launches" are not touched.
 * REFUSED with MGF_ERR_INVALID, nothing enqueued and nothing changed, in this order - ahead of the handle's contents: a NULL batch; a
 * negative n_ticks, iters, n_act, m or n_touch, in that order; n_ticks > 2^20; a mode other than MGF_ACTUATE_IMPULSE or
 * MGF_ACTUATE_FORCE; a touch_format other than MGF_ROLLOUT_TOUCH_FULL or MGF_ROLLOUT_TOUCH_SHORT; m > INT32_MAX; a byte count
 * (4 * n_ticks * n_act, then 64 * n_ticks * n_touch) that overflows int64_t - then the handle's own:
 * n_act != mgf_batch_actuator_count(b); n_touch != mgf_batch_touch_count(b) (report rows of the wrong length are a bug, not a prefix);
 * NULL u with n_act > 0 and n_ticks > 0; NULL touch with n_touch > 0 and n_ticks > 0; body == NULL with m > mgf_batch_len(b, -1).
 * n_ticks == 0: MGF_OK, nothing written, nothing enqueued beyond what mgf_batch_step(b, dt, iters, 0, stats) does.
 * OUT OF SCOPE here: ray sensors, feelers, zones or cameras per tick (they need the collider gather in the train) (since: Rollout sensor traces,
 * below - mgf_batch_rollout_observe writes the ray sensors' answers per tick, staged from the tick's own packed bodies, without the
 * gather; feelers, zones and cameras still not); sums over the
 * horizon (a reduction of the rows); the lone mgf_world; hipGraph capture. */
#define MGF_ROLLOUT_TOUCH_FULL  0   /* a row entry is mgf_touch_report, 64 bytes */
#define MGF_ROLLOUT_TOUCH_SHORT 1   /* 16 bytes: n_contacts, partner, normal_impulse, strongest_impulse of that report */
#define MGF_BATCH_ROLLOUT_TOUCH_LAUNCHES_PER_TICK 1  /* what the touch trace adds to a rollout's tick, in every pass that runs it */
typedef struct mgf_touch_short {
  int32_t n_contacts, partner;
  float normal_impulse, strongest_impulse;
} mgf_touch_short;                  /* 16 bytes: an entry of an MGF_ROLLOUT_TOUCH_SHORT row */
/* The host form: one upload (u and body), the device core, one download (the outputs given, the touch rows among them). */
MGF_API mgf_status mgf_batch_rollout_touches(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u, int64_t n_act, int32_t mode,
                                             const int32_t* body, int64_t m, float* x, float* q, float* v, float* omega,
                                             void* touch, int64_t n_touch, int32_t touch_format, mgf_step_stats* stats);
/* The same with u, body and the outputs in device memory (the device-pointer calls, above); stats stays host memory.  Also refused with
 * MGF_ERR_INVALID, nothing enqueued: a pointer that fails the look-up of the device-pointer calls for its full extent (mgf_batch_rollout_dev's,
 * and 64 * n_ticks * n_touch bytes of touch_dev - 16 * n_ticks * n_touch for MGF_ROLLOUT_TOUCH_SHORT), an output's bytes overlapping
 * another output's or an input's: touch_dev is held against x_dev, q_dev, v_dev, omega_dev, u_dev and body_dev. */
MGF_API mgf_status mgf_batch_rollout_touches_dev(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u_dev, int64_t n_act, int32_t mode,
                                                 const int32_t* body_dev, int64_t m, float* x_dev, float* q_dev, float* v_dev, float* omega_dev,
                                                 void* touch_dev, int64_t n_touch, int32_t touch_format, mgf_step_stats* stats);
/* ---- rollout sensor traces: the ray sensors' answers behind every tick of a rollout ----
 * A rollout records the state of chosen bodies behind every tick, and (rollout touch traces) what touched them.  What the agents SEE -
 * the ray-sensor rig of mgf_batch_set_sensors, the cheapest and most used observation of a batch - was still a loop of T casts with T
 * host waits.  These two calls are a rollout that can also write, behind tick t, row t of the contact sensors' reports and row t of the
 * ray sensors' answers.  The traces come in ONE struct, so that the next trace is a field and not another entry point.
 * THE DEFINITION is calls that exist, bit for bit.  With sensor[T][n_sensor] in the rig's order, the batch and every output are left as
 *   for t in 0 .. T-1:
 *     mgf_batch_apply_springs_dev(b, dt, NULL)                                                  (with a spring rig that is not empty)
 *     mgf_batch_actuate_dev(b, u[t], n_act, mode, NULL)                                        (skipped when n_act == 0)
 *     mgf_batch_step(b, dt, iters, 1, stats + t * n_worlds)
 *     mgf_batch_gather_state_dev(b, body, m, x[t], q[t], v[t], omega[t], NULL, NULL)           (skipped when m == 0)
 *     mgf_batch_read_touches_dev(b, touch + t * n_touch, n_touch)                              (with a touch trace)
 *     mgf_batch_cast_sensors_dev(b, sensor_mask, hits_row_t, NULL, n_sensor)                   (with a sensor trace)
 * leaves them.  sensor_format MGF_ROLLOUT_SENSOR_HIT: entry i of row t is hits_row_t[i], the 28-byte mgf_ray_hit.
 * MGF_ROLLOUT_SENSOR_DEPTH: an entry is one f32 - that hit's t, or the sensor's dt where nothing is hit (the depth cameras' rule: inf
 * for a sensor set with dt = inf; a sensor without a direction hits nothing).  EVERY entry of every row is written by a call that
 * returns MGF_OK.  The touch rows are mgf_batch_rollout_touches'.
 * A TRACE IS ASKED FOR by rows that are not NULL and a count that is not 0; then the count must be the rig's.  NULL rows, or a count
 * of 0, name no trace, whatever the rig holds (so a batch with a touch rig can trace its ray sensors alone); the formats and the reserved
 * words are checked all the same, the mask with a sensor trace alone (a zeroed struct with the touch fields set is in order).
 * traces == NULL: the call IS mgf_batch_rollout / _rollout_dev, launch for launch.  No sensor trace: it IS mgf_batch_rollout_touches /
 * _touches_dev with the struct's touch fields, launch for launch and byte for byte.  No touch trace: no launch of the touch trace.
 * ONE HOST WAIT per pass, as in a rollout.  NO COLLIDER GATHER rides in the train: behind a tick the tick's packed copy of the bodies is
 * what the gather would copy, and the cast stages from it.  A world whose tick t did not fit is undone and its row t is written in the
 * pass in which it completes t - never from a cast of an undone tick: the rows are written under the gate of the state rows.  (The
 * cast itself is not gated: a pass that runs a tick again casts for every world, and only the rows of the worlds that completed the
 * tick in this pass are written.)  The handle's scratch holds the cast (28 + 28 bytes a sensor); a cast call behind the rollout answers
 * as if the loop had run.
 * The trace adds MGF_BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK = 2 launches behind a tick in every pass that runs it - the cast, and the
 * rows with the obstacles of the sensors' worlds - whatever the worlds and the sensors, counted in "rollout_launches"; "query_launches"
 * and "drive_launches" are not touched.
 * REFUSED with MGF_ERR_INVALID, nothing enqueued and nothing changed, in this order - ahead of the handle's contents: a NULL batch; a
 * negative n_ticks, iters, n_act, m, n_touch or n_sensor, in that order; n_ticks > 2^20; a mode other than MGF_ACTUATE_IMPULSE or
 * MGF_ACTUATE_FORCE; a touch_format other than MGF_ROLLOUT_TOUCH_FULL or MGF_ROLLOUT_TOUCH_SHORT; a sensor_format other than
 * MGF_ROLLOUT_SENSOR_HIT or MGF_ROLLOUT_SENSOR_DEPTH; with a sensor trace a sensor_mask that a cast refuses (no bit, or one outside MGF_QUERY_ALL); a reserved word
 * that is not 0; m > INT32_MAX; a byte count (4 * n_ticks * n_act, then 64 * n_ticks * n_touch, then 28 * n_ticks * n_sensor - the
 * full records' bounds, whatever the formats) that overflows int64_t - then the handle's own: n_act != mgf_batch_actuator_count(b);
 * with a touch trace n_touch != mgf_batch_touch_count(b); with a sensor trace n_sensor != mgf_batch_sensor_count(b) (rows of the wrong
 * length are a bug, not a prefix); NULL u with n_act > 0 and n_ticks > 0; body == NULL with m > mgf_batch_len(b, -1); with a sensor
 * trace, a batch that holds bodies of several components - option "part_queries" or not: the cast in the train sees one collider a body.
 * n_ticks == 0: MGF_OK, nothing written, nothing enqueued beyond what mgf_batch_step(b, dt, iters, 0, stats) does.
 * OUT OF SCOPE here: feelers, zones and cameras per tick; batches with bodies of several components (the part-aware staging reads the
 * gathered colliders); the particles per tick; a kinds mask per sensor; the lone mgf_world; hipGraph capture. */
#define MGF_ROLLOUT_SENSOR_HIT   0   /* a row entry is mgf_ray_hit, 28 bytes */
#define MGF_ROLLOUT_SENSOR_DEPTH 1   /* one f32: the hit's t, or the sensor's dt where nothing is hit */
#define MGF_BATCH_ROLLOUT_SENSOR_LAUNCHES_PER_TICK 2   /* what the sensor trace adds to a rollout's tick, in every pass that runs it */
typedef void* mgf_trace_rows;            /* the rows of a trace: host memory for the host form, device memory for the device form */
typedef struct mgf_rollout_traces {      /* 64 bytes */
  mgf_trace_rows touch;  int64_t n_touch;    /* as mgf_batch_rollout_touches'; NULL or 0: no touch trace */
  mgf_trace_rows sensor; int64_t n_sensor;   /* [n_ticks][n_sensor] entries; NULL or 0: no sensor trace */
  int32_t touch_format, sensor_format, sensor_mask;   /* MGF_ROLLOUT_TOUCH_*, MGF_ROLLOUT_SENSOR_*, MGF_QUERY_* */
  int32_t reserved[5];                   /* must be 0 */
} mgf_rollout_traces;
/* The host form: one upload (u and body), the device core, one download (the outputs given, both traces' rows among them). */
MGF_API mgf_status mgf_batch_rollout_observe(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u, int64_t n_act, int32_t mode,
                                             const int32_t* body, int64_t m, float* x, float* q, float* v, float* omega,
                                             const mgf_rollout_traces* traces, mgf_step_stats* stats);
/* The same with u, body, the outputs and both trace pointers in device memory (the device-pointer calls, above); the struct itself and
 * stats stay host memory.  Also refused with MGF_ERR_INVALID, nothing enqueued: a pointer that fails the look-up of the device-pointer
 * calls for its full extent (mgf_batch_rollout_touches_dev's, and 28 * n_ticks * n_sensor bytes of traces->sensor - 4 * n_ticks *
 * n_sensor for MGF_ROLLOUT_SENSOR_DEPTH), an output's bytes overlapping another output's or an input's: the six outputs are held
 * against each other and against u_dev and body_dev. */
MGF_API mgf_status mgf_batch_rollout_observe_dev(mgf_batch* b, float dt, int32_t iters, int64_t n_ticks, const float* u_dev, int64_t n_act, int32_t mode,
                                                 const int32_t* body_dev, int64_t m, float* x_dev, float* q_dev, float* v_dev, float* omega_dev,
                                                 const mgf_rollout_traces* traces, mgf_step_stats* stats);
/* ---- slider joints between bodies: three angular rows, two off-axis rows, a limit, a motor and a lock, solved from the resident state ----
 * A gripper with parallel jaws, a lift, a telescopic leg, a suspension strut that stays on its axis, a piston - and, locked, a weld of
 * two bodies into one: a prismatic joint with a range and a drive, the tenth rig.  A spring cannot stand in for it (it needs a
 * stiffness the tick cannot carry and leaves five degrees of freedom open), and a hinge's free degree of freedom is the wrong one.
 * A slider ties `body` to `other` of one world, or to the world itself with other = -1:
 *   - three angular rows hold the frame of `other` onto the frame of `body`;
 *   - two linear rows hold other's anchor on the axis through body's anchor;
 *   - along that axis the anchor is free, or one of
 *       MGF_SLIDER_LIMIT  the travel d is held to [lo, hi];
 *       MGF_SLIDER_MOTOR  the relative speed along the axis is driven to a target from a table of the handle's, a row a call (a
 *                         rollout: a row a tick), the force capped at fmax;
 *       MGF_SLIDER_LOCK   the axis row is bilateral and holds d = lo: a fixed (weld) joint.  LOCK excludes the other two flags.
 * The reference has no joint, so this is the build's own definition, as the hinges are; no tick kernel changes and mgf_batch_step
 * applies no slider: the sliders are a pass of their own over the resident velocities.
 * A slider is a record (world, body, other, flags, pa, beta, pb, fmax, ax, lo, ua, hi, bx, pad0, ub, pad1): body and other indices
 * within world (other = -1: the far end is the world); pa, ax, ua the anchor, the unit slide axis and a unit reference perpendicular
 * to it in body's frame; pb, bx, ub the same in other's frame, or the world's; beta in [0, 1] the share of the position error removed
 * per call, used by the angular, off-axis, limit and lock rows; fmax >= 0 the motor's largest force (+inf allowed); lo <= hi the
 * travel range in length units; pad0 = pad1 = 0.  The travel is d = dot(Pb - Pa, A): other's anchor seen from body's along body's axis.
 * ONE CALL, mgf_batch_solve_sliders(b, h, iters, row, impulse_out), reads what mgf_batch_solve_joints reads of each end.  Every line
 * below is a separate rounded f32 operation, no fused multiply-add; rotate, cross, dot, M * v and invert are the ball joints' (above);
 * a sum of three terms is taken left to right; -x / y is (-x) / y; a vector times a scalar is (v.x * s, v.y * s, v.z * s).
 * SETUP, per slider i, from the state BEFORE the call:
 *   ra, rb, Pa, Pb, C = Pb - Pa, s = beta / h: the ball joint's lines, with this record's pa, pb and beta
 *   (other == -1: rb = 0, Pb = pb, im_b = 0, I_b = 0, v_b = omega_b = 0 and never written)
 *   A = rotate(q_a, ax);  T1 = rotate(q_a, ua);  T2 = cross(A, T1)
 *   other >= 0:  B = rotate(q_b, bx);  U1 = rotate(q_b, ub)
 *   other == -1: B = bx;  U1 = ub
 *   U2 = cross(B, U1);  ca = ra + C;  d = dot(C, A);  ims = im_a + im_b
 *   axis:     sA = cross(ca, A);  sB = cross(rb, A);  Km = (ims + dot(sA, I_a * sA)) + dot(sB, I_b * sB)
 *   off-axis: pA1 = cross(ca, T1);  pB1 = cross(rb, T1);  g1 = dot(C, T1) * s;  pA2 = cross(ca, T2);  pB2 = cross(rb, T2);  g2 = dot(C, T2) * s
 *             k11 = (ims + dot(pA1, I_a * pA1)) + dot(pB1, I_b * pB1);  k22 = (ims + dot(pA2, I_a * pA2)) + dot(pB2, I_b * pB2)
 *             k12 = dot(pA1, I_a * pA2) + dot(pB1, I_b * pB2);  k21 = dot(pA2, I_a * pA1) + dot(pB2, I_b * pB1)
 *             d2 = k11 * k22 - k12 * k21;  m11 = k22 / d2;  m12 = -k12 / d2;  m21 = -k21 / d2;  m22 = k11 / d2
 *   angular:  e = ((cross(A, B) + cross(T1, U1)) + cross(T2, U2)) * 0.5;  gw = e * s;  Kw = I_a + I_b (word by word);  Kwinv = invert(Kw)
 *   LOCK:                side = 2,  lb = (lo - d) * s
 *   LIMIT and d < lo:    side = -1, lb = (lo - d) * s
 *   LIMIT and d > hi:    side = +1, lb = -((d - hi) * s)
 *   otherwise:           side = 0, lb = 0    (the limit row is off for this call: a limit acts from the call after the travel passed it)
 *   MOTOR:  mmax = fmax * h;  w = entry i of the target table's row for this call (below)
 * A slider is SKIPPED on any of: d2 == 0; Km == 0 with any flag set; invert(Kw) failing (det == 0); a word of ra, rb, sA, sB, pA1, pA2,
 * pB1, pB2, g1, g2, gw, m11, m12, m21, m22, Km, Kwinv or lb not finite; with MOTOR a NaN mmax or a w that is not finite.  It is counted
 * in mgf_batch_counter "sliders_skipped" (cumulative; reading it waits for the stream), touches no velocity and reports zeros - and it
 * still takes its place in the order.
 * With  rate(n, a, b) = (dot(v_b - v_a, n) + dot(omega_b, b)) - dot(omega_a, a)  the update apply(n, a, b, lam) is
 *   v_a = v_a - n * (lam * im_a);  omega_a = omega_a - I_a * (a * lam)
 *   v_b = v_b + n * (lam * im_b);  omega_b = omega_b + I_b * (b * lam)      (other >= 0 only)
 * SWEEPS, iters times, over the sliders of a world in the order of the array given to mgf_batch_set_sliders; worlds are independent.
 * The rows of one slider in this order, each reading the current velocities (other == -1: v_b and omega_b are the zero vector and are
 * not written), am, al, aw, p1, p2 starting from 0 with the call:
 *   MOTOR:     lam = (w - rate(A, sA, sB)) / Km;  t = am + lam;  if (t < -mmax) t = -mmax;  if (t > mmax) t = mmax;  lam = t - am;  am = t
 *              apply(A, sA, sB, lam)
 *   side != 0: lam = (lb - rate(A, sA, sB)) / Km;  t = al + lam;  side == -1: if (t < 0) t = 0;  side == +1: if (t > 0) t = 0;  lam = t - al;  al = t
 *              apply(A, sA, sB, lam)
 *   angular:   L = -(Kwinv * ((omega_b - omega_a) + gw));  omega_a = omega_a - I_a * L;  omega_b = omega_b + I_b * L;  aw = aw + L
 *   off-axis:  r1 = rate(T1, pA1, pB1) + g1;  r2 = rate(T2, pA2, pB2) + g2;  l1 = -(m11 * r1 + m12 * r2);  l2 = -(m21 * r1 + m22 * r2)
 *              n = T1 * l1 + T2 * l2;  v_a = v_a - n * im_a;  omega_a = omega_a - I_a * (pA1 * l1 + pA2 * l2)
 *              v_b = v_b + n * im_b;  omega_b = omega_b + I_b * (pB1 * l1 + pB2 * l2);  p1 = p1 + l1;  p2 = p2 + l2
 * Nothing but v and omega is written; a body that no slider names is untouched to the bit, and so is a world that no slider names.
 * impulse_out is optional: when given, row i receives eight floats, (p1, p2, al, am, aw.x, aw.y, aw.z, 0) - the two off-axis
 * impulses, the limit's or the lock's, the motor's and the angular impulse over the call.  There is no warm start: no state is kept
 * between calls.  Sliders read no shapes: a batch with bodies of several components is answered.
 * THE TARGET TABLE.  The handle owns W[rows][mgf_batch_slider_count] floats in device memory: mgf_batch_set_slider_targets copies it
 * from host memory, mgf_batch_set_slider_targets_dev from device memory; a solve call names the row it reads.  Only sliders with MOTOR
 * read their column.  A motor with target 0 is a brake.  mgf_batch_set_sliders makes the table one row of zeros.
 * A call is MGF_BATCH_SLIDER_LAUNCHES = 1 launch, counted in "drive_launches", whatever the number of sliders and worlds: a workgroup
 * per world that has sliders, a lane per slider - hence at most MGF_BATCH_MAX_WORLD_SLIDERS = 256 sliders a world - which solves all
 * the rows of its slider as soon as both its bodies have been through the sliders listed ahead of it; no float atomic, and the result
 * does not depend on lane scheduling.
 * IN A ROLLOUT.  With a slider rig that is not empty, mgf_batch_rollout and its _dev, _touches and _observe forms become, bit for bit,
 * the loop
 *   [mgf_batch_apply_springs_dev(dt)] | mgf_batch_actuate_dev(u[t]) | [mgf_batch_solve_joints_dev(b, dt, iters, NULL)] |
 *   [mgf_batch_solve_hinges_dev(b, dt, iters, min(t, rows - 1), NULL)] | mgf_batch_solve_sliders_dev(b, dt, iters, min(t, rows - 1), NULL) |
 *   mgf_batch_step(dt, iters, 1) | mgf_batch_gather_state_dev(row t) | [traces]
 * - each table with its own rows.  Signatures, refusals and their order stay as they are; with an empty slider rig every call is
 * launch for launch what it was.  The sliders add MGF_BATCH_ROLLOUT_SLIDER_LAUNCHES_PER_TICK = 1 launch to a tick, counted in
 * "rollout_launches".  n_act == 0 with nothing traced is then NOT mgf_batch_step.  A world whose tick is undone and run again gets
 * tick t's sliders ONCE, and "sliders_skipped" counts as the loop's calls would.  mgf_batch_step itself stays World::step, launch for
 * launch: it applies no slider.
 * OUT OF SCOPE here: slider encoders - d, rate and side as a call and as a traced row (until then a caller forms d from
 * mgf_batch_gather_state) (since: Slider encoders, below - mgf_batch_read_sliders, mgf_batch_set_slider_trace); position (servo) motors; warm starting; sliders interleaved with hinges or with the contacts in one sweep;
 * more than MGF_BATCH_MAX_WORLD_SLIDERS sliders a world; sliders on the lone mgf_world; sliders inside mgf_batch_step. */
#define MGF_SLIDER_LIMIT 1  /* the travel along the axis is held to [lo, hi] */
#define MGF_SLIDER_MOTOR 2  /* the relative speed along the axis is driven to the table's target, the force capped at fmax */
#define MGF_SLIDER_LOCK 4   /* the axis row is bilateral and holds d = lo: a weld; excludes the other two */
#define MGF_BATCH_SLIDER_LAUNCHES 1  /* what one solve call adds to "drive_launches" */
#define MGF_BATCH_ROLLOUT_SLIDER_LAUNCHES_PER_TICK 1  /* what a slider rig that is not empty adds to a rollout's tick */
#define MGF_BATCH_MAX_WORLD_SLIDERS 256  /* sliders one world holds at most */
typedef struct mgf_batch_slider {
  int32_t world, body, other; uint32_t flags;   /* other = -1: the far end is the world; flags: MGF_SLIDER_LIMIT | MGF_SLIDER_MOTOR, or MGF_SLIDER_LOCK */
  mgf_vec3 pa; float beta;                      /* anchor in body's frame; Baumgarte share in [0, 1], used by the angular, off-axis, limit and lock rows */
  mgf_vec3 pb; float fmax;                      /* anchor in other's frame, or the world point; the motor's largest force, >= 0, +inf allowed */
  mgf_vec3 ax; float lo;                        /* slide axis in body's frame (unit); the lower end of the travel - with LOCK the travel held */
  mgf_vec3 ua; float hi;                        /* reference in body's frame, unit, perpendicular to ax; the upper end of the travel, >= lo */
  mgf_vec3 bx; float pad0;                      /* slide axis in other's frame, or the world's (unit); pad0 = 0 */
  mgf_vec3 ub; float pad1;                      /* reference in other's frame, or the world's, unit, perpendicular to bx; pad1 = 0 */
} mgf_batch_slider;                             /* 112 bytes: seven 16-byte words */
/* Replaces the rig by a copy of j[0 .. n); n = 0 clears it; the target table becomes one row of zeros.  No device work: the rig goes
 * up with the next call.  Refused with MGF_ERR_INVALID, the rig as it was ("the rig was not changed"), in this order: what
 * mgf_batch_set_joints refuses up to other == body, in its order; a flag bit beyond 7; MGF_SLIDER_LOCK together with MGF_SLIDER_LIMIT
 * or MGF_SLIDER_MOTOR; a word of the record that is not finite (fmax may be +inf); pad0 or pad1 not 0; beta outside [0, 1]; fmax < 0;
 * lo > hi; then, in double on the host, |ax|^2, |ua|^2, |bx|^2 or |ub|^2 more than 1e-3 away from 1; |dot(ax, ua)| or |dot(bx, ub)|
 * above 1e-3; last a world's slider beyond its MGF_BATCH_MAX_WORLD_SLIDERS-th.  The rig names (world, body) and (world, other):
 * mgf_batch_add_bodies and mgf_batch_add_compound_bodies afterwards leave every slider on the bodies it named.  Independent of the
 * other nine rigs. */
MGF_API mgf_status mgf_batch_set_sliders(mgf_batch* b, const mgf_batch_slider* j, int64_t n);
MGF_API int64_t    mgf_batch_slider_count(const mgf_batch* b);              /* -1 for NULL */
/* The target table replaced by a copy of w[rows][mgf_batch_slider_count] (host memory; one upload, waited for).  Refused with
 * MGF_ERR_INVALID, the table as it was, in this order: a NULL batch; rows < 1 or rows > 2^20; a NULL w with a rig that is not empty; a
 * byte count that overflows.  With an empty rig the number of rows is all that is kept. */
MGF_API mgf_status mgf_batch_set_slider_targets(mgf_batch* b, const float* w, int64_t rows);
/* The same from device memory (the device-pointer calls, above): a device-to-device copy enqueued on the context's stream and NOT
 * waited for - w_dev may be written again once the stream has passed the copy.  Also refused, nothing enqueued: a pointer that fails
 * the look-up of the device-pointer calls (4 * rows * mgf_batch_slider_count bytes of w_dev). */
MGF_API mgf_status mgf_batch_set_slider_targets_dev(mgf_batch* b, const float* w_dev, int64_t rows);
/* The sliders solved (above), the motors' targets from row `row` of the table.  Refused with MGF_ERR_INVALID, nothing enqueued and
 * nothing changed, in this order: a NULL batch, a non-finite h, iters < 0, row outside [0, rows).  iters == 0 or an empty rig: MGF_OK,
 * nothing enqueued, impulse_out not written.  Synchronous: one download where impulse_out is given (32 bytes a slider), one host wait.
 * MGF_ERR_HIP "internal error" behind the wait: a lane gave up waiting for its turn - a bug, never a wait for another workgroup; the
 * world's velocities are then as the call found them. */
MGF_API mgf_status mgf_batch_solve_sliders(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out);
/* The same with impulse_out in device memory (the device-pointer calls, above): enqueued on the context's stream and NOT waited for.
 * Also refused with MGF_ERR_INVALID, nothing enqueued: a pointer that fails the look-up of the device-pointer calls (32 bytes a
 * slider of impulse_out_dev). */
MGF_API mgf_status mgf_batch_solve_sliders_dev(mgf_batch* b, float h, int32_t iters, int64_t row, float* impulse_out_dev);
/* ---- slider encoders: travel, rate, limit side, off-axis gap and frame error of every slider, read from the resident state and traced per tick ----
 * Whoever drives a lift, a gripper jaw or a telescopic leg has to feel it: the travel d and its rate are the first two numbers a
 * controller reads of a prismatic joint, a planner's cost wants them - and the force the motor spent - at every tick of the horizon, and
 * whoever tunes beta and iters wants to know how far the far anchor leaves the axis and the two frames part under load.  A READING is
 * eight floats, 32 bytes,
 *   (d, rate, side, off1, off2, e.x, e.y, e.z)
 * formed from the state AS IT STANDS by the SETUP lines of the slider section above, verbatim, with the same helpers (rotate, cross,
 * dot); every line below is a separate rounded f32 operation, no fused multiply-add:
 *   ra, rb, Pa, Pb, C, A, T1, T2, B, U1: SETUP's lines (other == -1: B = bx, U1 = ub, Pb = pb, rb = 0, v_b = 0, omega_b = 0)
 *   U2 = cross(B, U1)
 *   ca = ra + C
 *   sA = cross(ca, A)
 *   sB = cross(rb, A)
 *   d = dot(C, A)                              the travel along the axis
 *   rate = (dot(v_b - v_a, A) + dot(omega_b, sB)) - dot(omega_a, sA)
 *                                              - rate(A, sA, sB) of the slider section: what the motor and axis rows of the NEXT solve see
 *   LOCK: side = 2.0f;  LIMIT and d < lo: side = -1.0f;  LIMIT and d > hi: side = +1.0f;  otherwise side = 0.0f
 *                                              - SETUP's flag rule: whether the NEXT solve's axis row would be on, and on which side
 *   off1 = dot(C, T1)
 *   off2 = dot(C, T2)                          the far anchor's distance from the axis: g1, g2 without the factor s
 *   e = ((cross(A, B) + cross(T1, U1)) + cross(T2, U2)) * 0.5      the frames' error: gw without the factor s
 * There is no division, no h and no beta: no slider is skipped and there is no counter.  Non-finite state gives non-finite words.  A
 * reading reads no shapes - a batch with bodies of several components is answered - and writes nothing but its output: the state is
 * untouched to the bit.
 * ONE CALL, mgf_batch_read_sliders(b, out), is MGF_BATCH_SLIDER_READ_LAUNCHES = 1 launch, counted in "drive_launches" as the solve's is:
 * a lane per slider by the caller's index over all worlds.  What set_many, mgf_batch_add_bodies or mgf_batch_set_sliders left on the
 * host goes up first, by the path the solve uses.
 * THE READINGS TABLE is the hinge encoders', kept apart from theirs: mgf_batch_set_slider_trace(b, rows, format) makes the handle
 * allocate and zero R[rows][mgf_batch_slider_count] entries in device memory; rows == 0 frees it and turns the trace off, which is the
 * default, and mgf_batch_set_sliders sets it back to 0 rows as it resets the target table.  An entry is
 *   MGF_SLIDER_TRACE_READING  32 bytes: the reading;
 *   MGF_SLIDER_TRACE_FULL     64 bytes: the reading, then the eight floats (p1, p2, al, am, aw.x, aw.y, aw.z, 0) of tick t's slider
 *                             solve - am / dt is the force the motor applied in tick t, al / dt the limit's or the lock's.
 * IN A ROLLOUT.  With a slider rig that is not empty and rows > 0, mgf_batch_rollout and its _dev, _touches, _touches_dev, _observe and
 * _observe_dev forms - no new entry point, no changed signature - are the defining loop of the slider section with one more line at the
 * end of tick t < rows:
 *   ... | mgf_batch_step(dt, iters, 1) | mgf_batch_gather_state_dev(row t) | [traces] | [mgf_batch_read_hinges_dev(b, row t)] | mgf_batch_read_sliders_dev(b, row t)
 * and every row is bit for bit what that loop gives; for FULL the impulse words are those of tick t's
 * mgf_batch_solve_sliders_dev(..., impulse_out) in that loop, and zeros with iters == 0, where no solve is enqueued.  Ticks t >= rows
 * write nothing and launch nothing - there is NO clamp: an output is never overwritten silently - and rows the call does not reach stay
 * as they were.  The trace adds MGF_BATCH_ROLLOUT_SLIDER_READ_LAUNCHES_PER_TICK = 1 launch to a tick that has a row, behind the hinge
 * trace's, counted in "rollout_launches"; with rows == 0 or an empty rig every rollout is launch for launch what it was.  A world
 * whose tick is undone and run again gets its row t in the pass in which it completes t, with the impulses of the pass that solved t.
 * mgf_batch_step traces nothing.
 * OUT OF SCOPE here: position (servo) motors; readings for ball joints; readings inside mgf_rollout_traces; a clamp or ring-buffer
 * mode of the table; the lone mgf_world; hipGraph capture. */
#define MGF_BATCH_SLIDER_READ_LAUNCHES 1  /* what one read call adds to "drive_launches" */
#define MGF_BATCH_ROLLOUT_SLIDER_READ_LAUNCHES_PER_TICK 1  /* what the sliders' readings table adds to a rollout's tick t < rows */
#define MGF_SLIDER_TRACE_READING 0  /* an entry of the table is the 32-byte reading */
#define MGF_SLIDER_TRACE_FULL 1     /* 64 bytes: the reading and the eight impulse words of the tick's slider solve */
typedef struct mgf_slider_reading {
  float d;         /* dot(C, A): the travel along the axis */
  float rate;      /* the rate of d as the next solve's motor and axis rows see it */
  float side;      /* 2: LOCK; -1 or +1: LIMIT is set and d is below lo or above hi - the next solve's axis row is on; 0: it is off */
  float off1, off2;  /* dot(C, T1), dot(C, T2): the far anchor's distance from the axis */
  mgf_vec3 e;      /* the frames' error, half the sum of the three cross products of the frames' vectors */
} mgf_slider_reading;  /* 32 bytes: two 16-byte words */
/* The readings of every slider into out[0 .. mgf_batch_slider_count) (host memory): one download, one host wait.  Refused with
 * MGF_ERR_INVALID, nothing enqueued, in this order: a NULL batch; a NULL out with a rig that is not empty.  An empty rig: MGF_OK,
 * nothing enqueued. */
MGF_API mgf_status mgf_batch_read_sliders(mgf_batch* b, mgf_slider_reading* out);
/* The same with out in device memory (the device-pointer calls, above): enqueued on the context's stream and NOT waited for.  Also
 * refused with MGF_ERR_INVALID, nothing enqueued: a pointer that fails the look-up of the device-pointer calls (32 bytes a slider of
 * out_dev), or that is not aligned to 16 bytes - the readings are stored as 16-byte words. */
MGF_API mgf_status mgf_batch_read_sliders_dev(mgf_batch* b, mgf_slider_reading* out_dev);
/* The readings table made rows x mgf_batch_slider_count entries of zeros in `format`; rows == 0: freed, no trace.  Refused with
 * MGF_ERR_INVALID, the table as it was, in this order: a NULL batch; rows < 0 or rows > 2^20; a format that is neither
 * MGF_SLIDER_TRACE_READING nor MGF_SLIDER_TRACE_FULL; a byte count that overflows.  With an empty rig rows and format are all that is kept. */
MGF_API mgf_status mgf_batch_set_slider_trace(mgf_batch* b, int64_t rows, int32_t format);
MGF_API int64_t    mgf_batch_slider_trace_rows(const mgf_batch* b);         /* -1 for NULL */
/* Rows [row0, row0 + n_rows) of the table into out (host memory, n_rows x mgf_batch_slider_count entries of 32 or 64 bytes): one
 * download, waited for.  Refused with MGF_ERR_INVALID, in this order: a NULL batch; row0 < 0; n_rows < 0; row0 + n_rows beyond the
 * table's rows; a NULL out with bytes to copy. */
MGF_API mgf_status mgf_batch_get_slider_trace(mgf_batch* b, void* out, int64_t row0, int64_t n_rows);
/* The same as a device-to-device copy, enqueued on the context's stream and NOT waited for.  Also refused, nothing enqueued: a pointer
 * that fails the look-up of the device-pointer calls. */
MGF_API mgf_status mgf_batch_get_slider_trace_dev(mgf_batch* b, void* out_dev, int64_t row0, int64_t n_rows);
/* name in {"launches_per_tick" (kernel launches one tick of the whole batch costs: 6, with or without obstacles; it does not grow with n_worlds), "capacity_retries",
 * "query_launches" (kernel launches of the last query call: it depends on neither n_worlds nor n), "query_run_ns" (HIP-event time of
 * the last query call's kernels, as mgf_world_counter's), "drive_launches" (kernel launches of the last mgf_batch_get_many / _set_many /
 * _set_forces / _apply_impulses / _copy_worlds call or device-pointer call on this batch - for a copy, on its destination: it depends on
 * neither n_worlds nor n), "device_skipped" (records of the device-pointer calls whose index was out of range, cumulative; waits for the
 * stream), "pair_table_uploads" (uploads of mgf_batch_copy_worlds_where's pair table, cumulative), "actuators_skipped" (above),
 * "rollout_launches" (launches of the last mgf_batch_rollout / _rollout_dev / _rollout_touches / _rollout_touches_dev call beyond its
 * ticks' own, the touch trace's one a tick a pass among them - and of the last mgf_batch_rollout_observe / _observe_dev call, the sensor trace's two a tick a pass among them), "springs_skipped" (above), "joints_skipped" (above), "hinges_skipped" (above), "sliders_skipped" (above)}. */
MGF_API mgf_status mgf_batch_counter(const mgf_batch* b, const char* name, int64_t* out);
/* Options (test knobs): "cons_per_body" [4] = the constraint records per body a world's share of the storage starts with (1 .. 4096); a
 * low value makes the first busy tick outgrow it, which the re-run path then handles.  "part_queries" [0] = 0 | 1 (any other value:
 * MGF_ERR_INVALID): rays, sweeps and box queries see the parts of bodies of several components (PART QUERIES, above); no device work. */
MGF_API mgf_status mgf_batch_set_option(mgf_batch* b, const char* key, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* MGF_HIP_H */
