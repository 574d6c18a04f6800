// Hand-written HIP kernels of the mgf per-tick hot path for gfx950 (wave64).
//
//   k_integrate<Tail>  RigidBodyVec::complete_motion + integrate (physics.rs:222-269), swept AABB
//                      (bounds.rs:60-68), fat-AABB refit test (world.rs:234-238).  In mgf_world_step (collide follows at
//                      once on the same bodies) its tail also lists each body's terrain faces (what k_terrain_rows does)
//                      and the blocks gather the scene bounds (what k_scene_bounds does; folded by k_zero_many); in the fused tick
//                      (r05) it also works out the body's Morton cell and rank over the previous tick's bounds (CellSort: no
//                      k_morton_count launch) and appends a 48-byte record of every body that lists a terrain face
//   k_scene_bounds / k_morton_count / k_scatter_leaves
//                      bodies counting-sorted into Morton cells (cell = 2L-bit prefix of the 30-bit code of the fat-box
//                      centre); the same kernels build the static grid over a terrain mesh's face boxes
//   k_scan<W>          the tick's prefix sums (cells, candidate rows, constraints per body): single pass, ticketed tiles, wave-wide
//                      decoupled look-back; its last thread checks the list capacities (caps_candidates / caps_constraints)
//   k_pair_brick       BVH::query (bvh.rs:283-310) of the world tree for every body at once: a brick of 4x4x4 Morton cells per
//                      block, the 8x8x8 cells around it staged in LDS, 8 lanes per query; queries that do not fit, and
//   k_pair_grid        the same by cell enumeration from global memory (the fallback, and what tiles with thin cells run);
//                      k_lbvh_low / k_lbvh_top + k_pair_rows (implicit 4-ary tree over the cells, cooperative walk)
//                      when one body spans too many cells; the hit SET is the reference's because acceptance is its own
//                      predicate on the leaf boxes
//   k_terrain_grid     Mesh::contacts' BVH::query by cell enumeration over the face boxes (row-major cells, bits per axis chosen
//                      from the mesh by build_face_grid: a heightfield's vertical axis gets none), hits stored as DFS ranks;
//                      k_terrain_rows = the walk of the flattened reference tree in the reference's order
//   k_candidates<FILL> the exact two-pass (count, fill) tree walk used when a candidate row overflows
//   k_rows_to_csr      rows -> CSR, terrain faces in DFS order (partner contacts are ordered by k_count_contacts)
//   k_narrow_pairs<A,B> / k_narrow_terrain<A>
//                      one kernel per shape-pair type over the candidate lists; pairs whose bounding spheres never come within
//                      reach leave first (comp_pair_far) and a block's survivors are packed into its first lanes
//   k_count_contacts / k_setup_pairs<SPHERES> (its first blocks: the terrain candidates, setup_terrain_one)
//                      Manifold::from + ContactConstraint::new (manifold.rs:120-148, solver.rs:101-191); in a world of
//                      spheres only the broadphase lists contacts (k_pair_grid<true> runs the sphere test) and
//                      k_setup_pairs<true> evaluates each one itself, so k_narrow_pairs is not launched
//   k_terrain_contacts / k_contacts_spheres (r05)
//                      a world of spheres over a small mesh, no candidate lists: the sphere-triangle tests of the bodies near the
//                      mesh (records from k_integrate's tail; a face by four lanes, tri_msphere_x4; as the last blocks of
//                      k_scatter_leaves_tc's launch), k_scan over p_cnt + tcn with the tick's counts in its epilogue
//                      (caps_contacts), then a block per 256 bodies: its partner contacts as an LDS list in canonical order,
//                      ContactConstraint::new for each
//   k_near_list / k_terrain_near<L> / k_terrain_tests / k_pair_grid_n<PARTS> / k_contacts_rows<false> / k_contacts_rows_parts (r06, k_front_rows.h)
//                      the same list-free front end for worlds that are NOT spheres only - capsules, mixed kinds, bodies of two
//                      components: the bodies near the mesh, their faces from the face grid with a cheap conservative reject
//                      (comp_tri_far) and a slot each, the body-triangle tests a lane per slot (on the context's second stream,
//                      beside the pair search); the pair search pools the accepted partners of a block's queries that may touch
//                      and runs the pair test - or the two-part manifold, raw contacts staged in LDS - a lane each, the rows
//                      hold contacts only; records from the rows.  k_contacts_rows<true> is r05's k_contacts_spheres.
//   k_contacts_rows_index<SPH> / k_contacts_rows_records<SPH> / k_flow6_links_records<SPH> (r07, option contacts_split)
//                      k_contacts_rows in two: ids, (a, b), degb / rev rows and the terrain contacts' records first; the partner contacts'
//                      records - what the solver's table kernels never read - as the last blocks of the links launch, or a launch of their own
//   k_contacts_rows_index_scan (r08, option scan_fused)
//                      k_contacts_rows_index<true> with the constraint numbering inside: no k_scan<1> over p_cnt + tcn ahead of it.  A
//                      workgroup of four groups of 256 bodies takes a ticket, publishes its run's total in a status word, lists its rows,
//                      and its first wave sums the totals of the runs before it (256 status words per sweep); the last ticket writes
//                      base[n] and the tick's counts (caps_contacts_pre / _post).  The other front ends keep the scan launch.
//   k_contacts_rows_index_tables (r09, option tables_fused)
//                      the same launch with a ticket per SOLVER BLOCK of a re-sorted store (a run of nb <= 1 024 body slots) and k_flow6_blocks'
//                      work for that block inside: the foreign partners into an LDS hash set and numbered ahead of the barrier that hands
//                      out the block's first id; binfo, bref, fbody / fcnt / nslots and both halves of every own F6Row from the owner, the
//                      partner, the counts and the exclusive prefix the numbering holds in LDS.  No k_flow6_blocks launch in such a tick
//   k_pair_wide (r06)  the few bodies whose fat box is far larger than the rest's (WideSpec, k_bodies.h: kept out of the scene
//                      bounds and rmax by k_integrate, never partners of the grid's pair search) find their partners-to-be
//                      from their own side: a workgroup per listed body
//   k_narrow_pairs_big / k_narrow_terrain_big (r06)
//                      worlds with a body of 5..32 components (its parts in the world's pool: Bodies::xl0): a wave per candidate pair of
//                      bodies, its lanes the part pairs in the oracle's order behind the bounding-sphere reject, the contacts packed in
//                      lane order into LDS and the pruner run by lane 0; a wave per (body, face), a lane per part behind comp_tri_far
//   k_tri_reject_batch the test entry mgf_tri_reject_batch: comp_tri_far's verdict beside the reference's contact count, per problem
//   k_solver_snapshot / k_solver_restore (r05)
//                      the velocities / impulses a persistent solver launch finds, and back, if it gives up (solver_abort_fallback)
//   k_chain_rows       order-preserving dependency links of the tick's constraint list (compact arrays, ConsLinks);
//   k_adj_fill / k_chain  the same for a caller-supplied list in any order (mgf_world_set_constraints)
//   k_flow6_blocks / k_flow6_links / k_flow6_chan
//                      block tables of the default solver: slots, foreign bodies, rows; the links along every body's chain
//                      written straight into the rows with their message channels; channel layout
//   k_solve_flow6      ContactConstraint::solve (solver.rs:203-252) for a whole Solver::solve call: one workgroup per spatial
//                      block, every body it touches, the arrival counters, the ready queue and the accumulated impulses in LDS,
//                      edges across block faces as 48-byte messages polled by one wave (solver mode 6, the default)
//   k_solve_flow5      ContactConstraint::solve (solver.rs:203-252) for a whole Solver::solve call: block-local persistent
//                      dataflow launch (a spatial block's velocities, arrival counters and ready queues in LDS)
//   k_solve_flow       the same graph with every hand-off through L2 (stand-by of k_solve_flow5, solver mode 1)
//   k_frontier0 / k_solve
//                      one launch per frontier of the unrolled (iterations x constraints) graph (solver mode 0, cross-check)
//   k_tile_select_* / k_export_bodies / k_import_ghosts / k_export_vel / k_import_ghost_vel / k_fetch_flags (k_tiles.h; batched in r05)
//                      the tile protocol: the boundary bodies and migrants of up to eight tiles per launch (per-block counts,
//                      offsets by one workgroup per tile, ordered scatter), 72-float ghost records out and in, the velocity refreshes
//                      between solver launches, every tile's solver flags into its pinned block; k_remove_positions_short /
//                      k_flag_* + k_compact_gather / _put: the stable compaction behind a hand-over; k_tick_snapshot: what a
//                      tile's tick changes, kept for the retry of a tick in which a persistent launch gave up
//   k_compound_* / k_bvh_raytrace / k_intersections_batch
//                      Compound (compound.rs:230-352), BVH::raytrace and Intersects (bvh.rs:345-369, collision.rs:169-373)
//   k_batch_front / _faces / _pairs / _pack / _setup / _solve (k_batch.h)
//                      a batch of small independent worlds (mgf_batch_*): the whole tick of one world by one workgroup per launch - integrate,
//                      the boxes and the pair search in LDS, the tests, the constraint records, Solver::solve with the bodies' records and
//                      progress counters in LDS
//   k_batch_parts_front / _faces / _obst / _pairs / _pack / _copy (k_batch_parts.h)
//                      for a batch that holds bodies of up to four components (mgf_batch_add_compound_bodies) five launches in the
//                      places of that tick's first four - seven a tick: the part in the candidate word, the obstacle candidates in a
//                      launch of their own (_obst), every part pair of a pair of bodies through the pruner and the manifold, up to 16
//                      records a pair; _setup and _solve follow unchanged.  The pruner is the lone world's, written once:
//                      parts_prune_n<SLOTS, BITS> (k_front_rows.h) serves k_pair_grid_n's four slots and _pairs' sixteen;
//                      k_narrow_pairs_parts<MP> (k_contacts.h) keeps its own in-place copy over global memory.  _copy: the part rows
//                      of a copied world
//   k_batch_query_gather / _ray / _sweep_bodies / _sweep_faces (k_batch_query.h)
//                      ray casts and sweeps against the worlds of a batch (mgf_batch_raycast_many / _sweep_many): a workgroup per (world,
//                      up to 256 queries; BatchWork), the world's colliders in LDS, 256 / count lanes a query and the best of them by
//                      bq_reduce, the mesh tree walked without a stack; the tests are k_query.h's
//   k_batch_observe_contacts / _overlap<FILL> (k_batch_observe.h)
//                      what else a caller reads of a batch every tick: the constraint list of every world folded per body
//                      (mgf_batch_read_body_contacts: a workgroup per world, the per-body ranges rebuilt in LDS, a lane per body walks its
//                      chain) and the bodies in a box (mgf_batch_overlap_aabb_many: the world's tight boxes in LDS, ballot-rank compaction).
//                      bo_front is that walk written once - the staging, the one barrier, the lane split, the ballot loop and a hit's
//                      rank - with the bodies' policy for a body's box, a loader for the box and a hook for what a hit stores: the
//                      overlap kernels', k_batch_zone_first's and k_batch_nearest's
//   k_batch_drive_get / _set<MODE> / _copy (k_batch_drive.h)
//                      acting on a batch between ticks: ConstrainedSet::get / set, the force and torque rows and impulses for any mix
//                      of (world, body) records (mgf_batch_get_many / _set_many / _set_forces / _apply_impulses: a lane per body the call
//                      names, its records in the caller's order from the host's stable sort) and world-to-world copies
//                      (mgf_batch_copy_worlds: a workgroup per pair, rows, packed copy, colliders and the constraint list in 16-byte words)
//   k_batch_dev_gather / _count / _fill / _apply<MODE, SEG> / _copy_where (k_batch_dev.h)
//                      the same for a caller whose arrays are device memory (mgf_batch_gather_state_dev / _set_many_dev / _set_forces_dev /
//                      _apply_impulses_dev / _copy_worlds_where): bodies by their flat index, every index checked on the device, records
//                      that name a body twice put in order per body on the device (counts by integer atomics, the library's prefix sum,
//                      a lane per body sorts its segment) and applied by k_batch_drive_set's own apply step; the copy of the pairs a
//                      device mask selects
//   k_batch_query_plan_count<WORDS> / _plan_cut / _plan_fill, k_batch_query_ray_dev<SRC> / _sweep_bodies_dev<SRC> (k_batch_query_dev.h)
//                      ray casts and sweeps for a caller whose queries and hits are device memory (mgf_batch_raycast_many_dev /
//                      _sweep_many_dev): the sort by world built on the device (ranks by integer atomics, the library's prefix sums,
//                      work items of up to 256 queries), every world index and tag checked there; then k_batch_query.h's own code
//                      with the work item from that table, or - a fixed number of queries a world - from blockIdx.x by arithmetic
//   k_batch_sensor_ray (k_batch_sensor.h)
//                      ray sensors fixed in the frame of a body (mgf_batch_set_sensors / _cast_sensors / _cast_sensors_dev): the rig sorted
//                      by world and cut into work items on the host, once; a cast reads the bodies' x and q, forms every sensor's particle
//                      P = x + rotate(q, p), D = rotate(q, d) and casts it through bq_ray_front (k_batch_query.h), k_batch_query_ray's front
//   k_batch_camera_tile / _depth (k_batch_camera.h)
//                      depth cameras fixed in the frame of a body (mgf_batch_set_cameras / _cast_cameras / _cast_cameras_dev): a workgroup per
//                      tile of 16 x 16 pixels, a lane per pixel; the tile bounds its rays by a cone and a length, drops every body whose
//                      padded sphere lies outside both, compacts the survivors into LDS, and every pixel runs k_batch_query_ray's loop over
//                      them alone; _depth writes the depth image behind the obstacle pass
//   k_batch_zone_first<SRC> (k_batch_zone.h)
//                      box zones fixed in the frame of a body or of the world (mgf_batch_set_zones / _read_zones / _read_zones_dev), and
//                      the caller's own boxes from device memory (mgf_batch_overlap_first_dev): per box the count and the first k bodies,
//                      a record of fixed width - through bo_front (k_batch_observe.h), k_batch_observe_overlap's front, with the ignored
//                      body on: count and fill in one pass, no total, no host wait
//   k_batch_nearest<SRC> (k_batch_nearest.h)
//                      the same zones and boxes, nearest first (mgf_batch_read_zones_nearest / _read_zones_nearest_dev /
//                      _overlap_nearest_dev): per box the count and the k <= 32 nearest bodies by the squared distance of their tight
//                      box's centre from the box's, ties by index, and those distances where asked for - the count through bo_front,
//                      then k rounds of selection over the staged boxes: a lane's least 64-bit key (bits(d2) << 32) | index above the
//                      last one chosen, min-reduced over the zone's lanes by __shfl_xor; one launch, no sort, no atomic
//   k_batch_touch (k_batch_touch.h)
//                      contact sensors (mgf_batch_set_touches / _read_touches / _read_touches_dev): per (body, partner filter) the last
//                      tick's constraint list folded in the body's chain order - count, net normal impulse, sum of the normal impulses -
//                      and the strongest matching record's partner, index, direction and arm; a lane per sensor, the ranges of `a` by
//                      binary search, the list's `b` column through LDS a tile at a time for the filters that need a body's `b`
//                      occurrences; nothing built in global memory, one launch, no atomic
//   k_batch_feeler_bodies (k_batch_feeler.h)
//                      feelers fixed in the frame of a body (mgf_batch_set_feelers / _cast_feelers / _cast_feelers_dev): a sphere or
//                      capsule with a displacement - or the body's own resident collider - formed from the bodies' x and q, P = x +
//                      rotate(q, p), D = rotate(q, d), delta turned by q or kept in world coordinates, and swept against the world's
//                      staged colliders through bq_sweep_front (k_batch_query.h), k_batch_query_sweep_bodies' front; the cast is always
//                      stored, and k_batch_query_sweep_faces / _sweep_obstacles take it up again from there
//   k_batch_actuate<MODE, OUT> (k_batch_actuator.h)
//                      actuators fixed in the frame of a body (mgf_batch_set_actuators / _actuate / _actuate_dev): a lane per run of one
//                      body's actuators, sorted on the host when the rig is set; per actuator s = gain * clamp(u), the direction and
//                      the arm turned by the body's q, the wrench (L, A) = (e s, cross(r, L)) or a pure couple, applied in the caller's
//                      order with batch_drive_apply's arithmetic - an impulse, or added to the force and torque rows; no float atomic
//   k_batch_rollout_act<MODE> / k_batch_rollout_record (k_batch_rollout.h)
//                      a rollout's two launches a tick inside the step's launch train (mgf_batch_rollout / _rollout_dev): k_batch_actuate's
//                      walk on row t of the controls ahead of tick t's launches, k_batch_dev_gather's rows into row t of the traces
//                      behind them - both under the train's gate done[k] == tick, and a word `act` beside `done` that keeps a world
//                      whose tick is undone and run again from being actuated twice; record advances it, a lane per world
//   k_batch_spring_wrench / k_batch_spring_apply<GATED> (k_batch_spring.h)
//                      spring-dampers between two body-fixed points, or one and a point of the world (mgf_batch_set_springs /
//                      _apply_springs / _apply_springs_dev, and ahead of every tick of a rollout): a lane per spring forms the
//                      impulses on both ends from the state before the call - lengths, point velocities, a clamp, two cross
//                      products - into the handle's buffer; then a lane per run of one body's ends, sorted on the host when the rig
//                      is set, applies them in list order with batch_drive_apply's arithmetic; no float atomic.  GATED: under the
//                      rollout train's gate done[k] == tick && act[k] == tick, folded into the run length
//   batch_joint_loop<Rows, GATED> (k_batch_joint_loop.h) - no kernel: the skeleton of the three joint solvers below, each of which is
//                      one call of it - the gate, the slots' load, the plan's words, the dataflow loop with its bounded spin, the
//                      store-back and the impulse row - over a Rows type that holds the kind's registers, setup, rows and store
//   k_batch_joint_solve<GATED> (k_batch_joint.h)
//                      ball joints between two body-fixed points, or one and a point of the world (mgf_batch_set_joints /
//                      _solve_joints / _solve_joints_dev, and between the actuation and the tick of a rollout): sequential impulses
//                      over the resident velocities - a workgroup per world, a lane per joint; the lane keeps its joint's arms, bias
//                      and inverse K in registers, the world's jointed bodies sit in LDS slots, and the sweeps run in list order by
//                      k_batch_solve's dataflow over ranks and degrees the host planned; bounded spin, no float atomic.  GATED:
//                      under the rollout train's gate done[k] == tick && act[k] == tick, the workgroup's early return
//   k_batch_hinge_solve<GATED> (k_batch_hinge.h)
//                      hinge joints (mgf_batch_set_hinges / _set_hinge_targets / _solve_hinges / _solve_hinges_dev, and behind the
//                      ball joints of a rollout's tick): k_batch_joint_solve's launch with four rows a hinge - a velocity motor with
//                      a torque cap, a limit of the hinge angle, two angular rows that keep the axes parallel, the point - solved in
//                      one turn of the lane with both bodies' velocities in registers; the same plan, slots, dataflow, bounded spin
//                      and gate; the motors' targets from a row of the handle's table
//   k_batch_slider_solve<GATED> (k_batch_slider.h)
//                      slider joints (mgf_batch_set_sliders / _set_slider_targets / _solve_sliders / _solve_sliders_dev, and behind the
//                      hinges of a rollout's tick): k_batch_hinge_solve's launch with the rows of a slider - a velocity motor with a
//                      force cap along the axis, a limit of the travel or a lock, three angular rows that hold the two frames
//                      together, two linear rows that hold the anchor on the axis - solved in one turn of the lane with both
//                      bodies' velocities in registers; the same plan, slots, dataflow, bounded spin and gate; the motors' targets
//                      from a row of the handle's table
//   batch_joint_read<Reading, GATED, FORMAT> (k_batch_joint_read.h; the frame lines in k_batch_hinge_frame.h) - no kernel: the skeleton
//                      of the two encoders below, each of which is one call of it - a lane per joint by the caller's index loads the
//                      record and both ends, forms the SETUP frames from the state as it stands, takes the entry's two words from
//                      the kind's Reading and writes them - 32 bytes, or 64 with the eight impulse words of the tick's solve behind
//                      them - with float4 stores; no plan, no LDS, no division, no atomic, nothing written but the output.  GATED:
//                      the traces' gate done[k] == t + 1 && act[k] <= t + 1, the lane's own, ahead of every load of state
//   k_batch_read_hinges<GATED, FORMAT> (k_batch_hinge_read.h)
//                      hinge encoders (mgf_batch_read_hinges / _read_hinges_dev, and behind the record of every tick of a rollout that
//                      has a row in the readings table - mgf_batch_set_hinge_trace): (c, sn, rate, side, gap, tilt2) a hinge
//   k_batch_read_sliders<GATED, FORMAT> (k_batch_slider_read.h)
//                      slider encoders (mgf_batch_read_sliders / _read_sliders_dev, and behind the hinge trace's launch of every tick
//                      that has a row in the sliders' table - mgf_batch_set_slider_trace): (d, rate, side, off1, off2, e) a slider,
//                      with two loads of its own for the ends' linear velocities
//   k_batch_trace_touch<FORMAT> (k_batch_trace.h)
//                      the touch trace of a rollout (mgf_batch_rollout_touches / _touches_dev): k_batch_touch's fold of every world's
//                      list behind tick t into row t of the reports, one launch a tick behind k_batch_rollout_record; the train's gate
//                      done[k] == t + 1 && act[k] <= t + 1 is the workgroup's and is folded into the item's count and the list's
//                      length; a full report of 64 bytes or a short one of 16
//   k_batch_scan_rays / k_batch_scan_rows<FORMAT> (k_batch_scan.h)
//                      the sensor trace of a rollout (mgf_batch_rollout_observe / _observe_dev): two launches a tick behind the touch
//                      trace's.  The ray sensors' cast - bs_rays over TickBodies, the policy that stages a world's bodies from bpk,
//                      the tick's packed copy, so no collider gather rides in the train - into the handle's scratch, ungated; then a
//                      lane per sensor under the train's gate done[k] == t + 1 && act[k] <= t + 1 takes the record up, puts the
//                      stored particle through its world's obstacles and writes row t: the 28-byte hit, or the depth alone
//   k_batch_pq_ray<SRC> / _sweep<SRC> / _sensor / _feeler / _overlap<FILL> / _zone<SRC> / _nearest<SRC> (k_batch_part_query.h)
//                      the body passes of the rays, sweeps, sensors, feelers, box overlaps and zones of a batch that holds bodies of
//                      several components, under option "part_queries": the fronts and bodies of the kernels above - each written
//                      once, over a policy of what the bodies of a world are (PlainBodies, k_batch_query.h) - with the policy that
//                      sees parts (PartBodies): every part of
//                      every body through the single-shape test (`part` of a hit), a reject sphere per body of several parts staged
//                      beside the colliders, the parts read from wp0 / wp1 for the bodies that survive it, `part` carried through
//                      the reduction (PartBest); a body's box the union of its parts' bounds.  The passes behind them are unchanged
//   k_query_* (k_query.h) ray casts, sweeps and box overlaps against the world's bodies, terrain and obstacles between ticks, over a grid
//                      of the bodies' current tight boxes built per call (never the tick's lists).  k_query.h is also where every test
//                      and record of a query is written once, for the world's kernels and the batch's: to_comp(float4, float4), the
//                      terrain's node and face tests (q_ray_terrain / q_sweep_terrain<Mesh> over q_mesh_walk), q_ray_store / q_sweep_store /
//                      q_sweep_load, the candidates QueryBest / SweepBest with what bq_reduce needs of them, and the grid walk's
//                      q_clip / q_next_crossing
//
// All f32 arithmetic follows the reference's operation order; the TU is built with
// -ffp-contract=off.
#pragma once
// The kernels live in the k_*.h parts, each including the one before it:
//   k_bodies.h -> k_broadphase.h -> k_contacts.h -> k_front_rows.h -> k_links.h -> k_solver_flow.h -> k_tiles.h -> k_api.h
#include "k_api.h"
#include "k_query.h"  // the world queries between ticks (k_query_*), beside the tick
#include "k_batch.h"  // many small worlds, a workgroup each (k_batch_*), beside the one-world tick
#include "k_batch_parts.h"  // the same tick for bodies of up to four components (k_batch_parts_*)
#include "k_batch_query.h"  // the queries of k_query.h for the worlds of a batch (k_batch_query_*)
#include "k_batch_observe.h"  // per-body contact summaries and box overlaps of a batch (k_batch_observe_*)
#include "k_batch_drive.h"  // get / set, forces, impulses and world copies of a batch (k_batch_drive_*)
#include "k_batch_dev.h"  // the same from and into the caller's device memory (k_batch_dev_*)
#include "k_batch_query_dev.h"  // ray casts and sweeps from and into the caller's device memory (k_batch_query_plan_*, k_batch_query_*_dev)
#include "k_batch_sensor.h"  // ray sensors fixed in the frame of a body, cast from the resident poses (k_batch_sensor_ray)
#include "k_batch_camera.h"  // depth cameras fixed in the frame of a body, a workgroup per image tile (k_batch_camera_*)
#include "k_batch_zone.h"  // box zones: the count and the first k bodies of every box, a fixed-width record (k_batch_zone_first)
#include "k_batch_nearest.h"  // box zones, nearest first: the count and the k nearest bodies of every box (k_batch_nearest)
#include "k_batch_touch.h"  // contact sensors: the constraint list folded per (body, partner), a fixed-width report (k_batch_touch)
#include "k_batch_feeler.h"  // feelers: spheres and capsules fixed in the frame of a body, swept from the resident poses (k_batch_feeler_bodies)
#include "k_batch_actuator.h"  // actuators: wrenches formed from the resident poses and applied, a lane per body (k_batch_actuate)
#include "k_batch_rollout.h"  // rollouts: a row of controls ahead of every tick of a step call, a row of state behind it (k_batch_rollout_act, _record)
#include "k_batch_spring.h"  // springs between bodies: impulses formed from the resident state, applied a lane per body (k_batch_spring_wrench, _apply)
#include "k_batch_joint_loop.h"  // the joint solvers' skeleton: one launch shape and one dataflow loop over a Rows type (batch_joint_loop)
#include "k_batch_joint.h"  // ball joints between bodies: sequential impulses over the resident velocities, a workgroup per world (k_batch_joint_solve)
#include "k_batch_hinge.h"  // hinge joints between bodies: the joints' launch with motor, limit, angular and point rows (k_batch_hinge_solve)
#include "k_batch_slider.h"  // slider joints between bodies: the hinges' launch with motor, axis, angular and off-axis rows (k_batch_slider_solve)
#include "k_batch_joint_read.h"  // the encoders' skeleton: one lane's walk, gate, loads and stores over a Reading type (batch_joint_read)
#include "k_batch_hinge_read.h"  // hinge encoders: angle, rate, limit side, gap and tilt from the resident state, a lane per hinge (k_batch_read_hinges)
#include "k_batch_slider_read.h"  // slider encoders: travel, rate, limit side, off-axis gap and frame error from the resident state, a lane per slider (k_batch_read_sliders)
#include "k_batch_part_query.h"  // rays, sweeps and box queries that see the parts of bodies of several components (k_batch_pq_*)
#include "k_batch_trace.h"  // the touch trace of a rollout: the contact sensors' reports behind every tick (k_batch_trace_touch)
#include "k_batch_scan.h"  // the sensor trace of a rollout: the ray sensors' answers behind every tick (k_batch_scan_rays, _rows)
