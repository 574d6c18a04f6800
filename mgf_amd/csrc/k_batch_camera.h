// Body-mounted depth cameras of a batch (mgf_batch_set_cameras, mgf_batch_cast_cameras, mgf_batch_cast_cameras_dev; host_batch_camera.inc).
// (Part of the kernel set described in kernels.h.)
//
// A camera is a record fixed in the frame of a body: (world, body, p, r, tan_x, tan_y, far, width, height, flags).  It looks along +z of
// its own frame, +x to the right, +y up; pixel (ix, iy) - row iy from the top, column ix from the left - has the direction
//   u = ((float)(2 ix + 1) / (float)width - 1) * tan_x      v = (1 - (float)(2 iy + 1) / (float)height) * tan_y      d_cam = (u, v, 1)
// and the particle, with x and q the body's rows as for a sensor (k_batch_sensor.h: x WITHOUT delta),
//   P = x + rotate(q, p)      D = rotate(q, rotate(r, d_cam))      dt = far
// every operation a separate f32 one.  Its answer is what k_batch_query_ray writes for that particle against that world, with `body`
// ignored if MGF_SENSOR_IGNORE_SELF is set; its depth is that hit's t, or far where nothing is hit.
//   k_batch_camera_tile   a workgroup per tile of kCamTileW x kCamTileH pixels of one camera (the tile table is built on the host when the
//                         rig is set), a lane per pixel.  The pixels of a tile leave one point in nearly one direction, so the tile
//                         settles once which bodies any of them can meet:
//                         1. every lane forms P (uniform) and its own D; the tile's cone - the axis through the middle of the tile's
//                            rectangle on the plane z = 1, the smallest cosine to it and the largest |D| among the rectangle's four corners
//                            (both extremes over a rectangle are taken at a corner: D is linear in (u, v) and a cone of less than a right
//                            angle is convex) - follows from the record and the body's rows alone;
//                         2. every live lane holds ITS OWN D against the cone and the length; a lane that is outside, or whose |D|^2 is
//                            below bq_ray_far's 1e-30, or NaN, switches the cull off for the whole tile (s_ctl[1]);
//                         3. the lanes stride over the world's col0 / col1: the ignored body is dropped, and with the cull on a body
//                            whose padded sphere lies wholly outside the cone or wholly beyond far * max |D| (cam_outside); the survivors
//                            are compacted into dynamic LDS with their index - a wave ballot, one integer LDS add a wave;
//                         4. every live lane runs bq_ray_item's loop over the survivors only - bq_ray_far, q_ray_comp, QueryBest::offer,
//                            which ranks totally: the order of the survivors changes nothing - walks the terrain and stores the depth
//                            and, where there is somewhere to store them, the hit, the particle and the pixel's world.
//                         No bq_reduce: a pixel has one lane.  No lane leaves ahead of a __syncthreads: there is no return at all.
//   k_batch_camera_depth  a lane per pixel behind the obstacle pass: the depth from the final hit record and the stored particle's dt
// The obstacles are k_batch_query_ray_obstacles' (k_batch_query.h), unchanged, over the stored particles and the stored worlds.
// The cull is conservative (DESIGN.md 8b has the argument): cam_outside returns true only where the body's sphere of radius
// sqrt(lim^2 + 1e-4 |w|^2) - exactly the square bq_ray_far compares with - padded by another 1 % is farther than that from every point
// P + s D, s in [0, far], D in the cone; bq_ray_far is then true for every pixel of the tile.  -DMGF_CAMERA_CULL=0 compiles the cull out
// (tools/build_variant.sh; tools/batch_camera_bench.py times both).
#pragma once
#include "k_batch_query.h"

#ifndef MGF_CAMERA_CULL
#define MGF_CAMERA_CULL 1
#endif

namespace mgf {

constexpr uint32_t kCamTileW = 16, kCamTileH = 16;
static_assert(kCamTileW * kCamTileH == (uint32_t)kBatchBlock, "a lane per pixel of a tile");
constexpr float kCamMinCos = 0.05f;  // a tile whose cone is wider than this cosine (or NaN) is culled by distance alone

struct CameraIn { int32_t world, body; float p[3], r[4], tan_x, tan_y, far; int32_t width, height, flags, reserved; };  // mgf_batch_camera
static_assert(sizeof(CameraIn) == 64, "the rig goes up as the caller's records");

struct BatchCameraArgs {
  const float4* col0;     // the persistent colliders of every world's bodies, world k at [w_off[k], w_off[k + 1])
  const float4* col1;
  const uint32_t* w_off;
  BatchTerrains T;
  const float4* x;        // the bodies' rows (Bodies::x, ::q)
  const float4* q;
  const CameraIn* cams;   // world and body checked on the host
  const uint4* tiles;     // (camera, the camera's first pixel, x0 | y0 << 16, -)
  int32_t mask;
  float* depth;           // by pixel; null: not stored (the depth pass behind the obstacles writes it)
  int32_t* out;           // by pixel: 7 words (mgf_ray_hit); null: not stored
  float* parts;           // by pixel: 7 words (mgf_particle); null: not stored
  int32_t* world;         // by pixel: the camera's world, for the obstacle pass; null: not stored
};

__device__ __forceinline__ V3 cam_dir(const CameraIn& c, uint32_t ix, uint32_t iy) {
  const float u = ((float)(2u * ix + 1u) / (float)c.width - 1.0f) * c.tan_x;
  const float v = (1.0f - (float)(2u * iy + 1u) / (float)c.height) * c.tan_y;
  return mk3(u, v, 1.0f);
}

// Is the body farther than its padded sphere from every point p + s D with D in the cone (unit axis ax, cosine >= cs, sine <= sn) and
// |s D| <= reach?  The sphere is bq_ray_far's - centre, R * 1.01 + 1e-3, and the 1e-4 |w|^2 of its comparison - times 1.01.  The cone's
// distance from below: in the plane through the axis and the centre the cone is a wedge inside the half plane perp cs - al sn <= 0, and
// behind the eye inside al >= 0.  (NaN anywhere: every comparison is false - not outside.  A sphere that holds the eye: |w| < pad.)
__device__ __forceinline__ bool cam_outside(float4 a, float4 b, V3 p, V3 ax, float cs, float sn, float reach) {
  const bool sph = (int)f2u(b.w) == KIND_SPHERE;
  const V3 bd = xyz(b);
  const V3 c = sph ? xyz(a) : xyz(a) + bd * 0.5f;
  const float R = sph ? a.w : a.w + 0.5f * mag(bd);
  const V3 w = c - p;
  const float lim = R * 1.01f + 1e-3f, l2 = dot(w, w);
  const float pad = __builtin_sqrtf(lim * lim + 1e-4f * l2) * 1.01f;
  if (__builtin_sqrtf(l2) - pad > reach) return true;
  if (!(cs > kCamMinCos)) return false;
  const float al = dot(w, ax), perp = mag(cross(w, ax));
  const float gap = al >= 0.0f ? perp * cs - al * sn : fmaxf(-al, perp * cs);
  return gap > pad;
}

// LDS (dynamic): 36 bytes a body - col0, col1, index of the survivors - and four words (survivors, cull off, -, -).
__global__ __launch_bounds__(kBatchBlock) void k_batch_camera_tile(BatchCameraArgs A) {
  extern __shared__ float4 s_dyn[];
  const uint4 it = A.tiles[blockIdx.x];
  const CameraIn c = A.cams[it.x];  // (wave-uniform loads)
  const uint32_t g0 = A.w_off[(uint32_t)c.world];
  const uint32_t n = (A.mask & MGF_QUERY_BODIES) ? A.w_off[(uint32_t)c.world + 1u] - g0 : 0u;
  float4 *s_c0 = s_dyn, *s_c1 = s_dyn + n;
  uint32_t* s_idx = reinterpret_cast<uint32_t*>(s_dyn + 2 * (size_t)n);
  uint32_t* s_ctl = s_idx + n;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t x0 = it.z & 0xFFFFu, y0 = it.z >> 16;
  const uint32_t ix = x0 + (threadIdx.x % kCamTileW), iy = y0 + (threadIdx.x / kCamTileW);
  const bool live = ix < (uint32_t)c.width && iy < (uint32_t)c.height;
  if (threadIdx.x == 0u) { s_ctl[0] = 0u; s_ctl[1] = 0u; }
  __syncthreads();
  // the particle, exactly as defined
  const size_t g = (size_t)g0 + (uint32_t)c.body;
  const float4 bx = A.x[g], bq = A.q[g];
  const Quat rot = mkq(bq.x, mk3(bq.y, bq.z, bq.w)), rc = mkq(c.r[0], mk3(c.r[1], c.r[2], c.r[3]));
  const V3 p = xyz(bx) + rotate(rot, ld3(c.p));
  const float dt = c.far;
  const int32_t ign = (c.flags & MGF_SENSOR_IGNORE_SELF) ? c.body : -1;
  V3 d = mk3(0.0f, 0.0f, 0.0f);
  int32_t mask = 0;
  if (live) {
    d = rotate(rot, rotate(rc, cam_dir(c, ix, iy)));
    mask = A.mask;
    if (!q_ray_castable(d)) mask = 0;  // (no direction, or one outside the band: no hit, by definition - k_query.h)
  }
  const float dd = dot(d, d);
  // the tile's cone, from the corners of its live rectangle (uniform)
  V3 ax = mk3(0.0f, 0.0f, 0.0f);
  float cs = 0.0f, sn = 1.0f, reach = kInf;
  if (MGF_CAMERA_CULL && n) {
    const uint32_t x1 = min(x0 + kCamTileW, (uint32_t)c.width) - 1u, y1 = min(y0 + kCamTileH, (uint32_t)c.height) - 1u;
    const V3 k00 = cam_dir(c, x0, y0), k11 = cam_dir(c, x1, y1);
    const V3 mid = rotate(rot, rotate(rc, mk3(0.5f * (k00.x + k11.x), 0.5f * (k00.y + k11.y), 1.0f)));
    ax = mid * (1.0f / mag(mid));
    float c0 = 1.0f, dmax = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const V3 ck = rotate(rot, rotate(rc, mk3((k & 1) ? k11.x : k00.x, (k & 2) ? k11.y : k00.y, 1.0f)));
      const float lk = mag(ck);
      c0 = fminf(c0, dot(ck, ax) / lk);
      dmax = fmaxf(dmax, lk);
    }
    dmax *= 1.001f;
    cs = c0 * 0.999f - 1e-3f;
    sn = __builtin_sqrtf(fmaxf(1.0f - cs * cs, 0.0f)) * 1.001f;
    reach = dt * dmax;
    // every pixel answers for itself: inside a cone half as padded, no longer than dmax, and long enough for bq_ray_far to reject at all
    const float len = __builtin_sqrtf(dd);
    const bool bad = live && !(dd >= 1e-30f && dot(d, ax) >= (c0 * 0.9995f - 5e-4f) * len && len <= dmax);
    const unsigned long long any = __ballot(bad);
    if (any != 0ull && lane == 0u) s_ctl[1] = 1u;
  }
  __syncthreads();
  const bool cull = MGF_CAMERA_CULL && s_ctl[1] == 0u;
  // cull and stage: every lane makes every trip
  for (uint32_t base = 0; base < n; base += kBatchBlock) {
    const uint32_t i = base + threadIdx.x;
    bool keep = i < n && (int32_t)i != ign;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
    if (keep) {
      a = A.col0[(size_t)g0 + i]; b = A.col1[(size_t)g0 + i];
      if (cull && cam_outside(a, b, p, ax, cs, sn, reach)) keep = false;
    }
    const unsigned long long m = __ballot(keep);
    uint32_t at = 0u;
    if (lane == 0u && m != 0ull) at = atomicAdd(&s_ctl[0], (uint32_t)__popcll(m));
    at = (uint32_t)__shfl((int)at, 0);
    if (keep) {
      const uint32_t r = at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      s_c0[r] = a; s_c1[r] = b; s_idx[r] = i;
    }
  }
  __syncthreads();
  const uint32_t m = s_ctl[0];
  QueryBest best;
  if (mask & MGF_QUERY_BODIES) {
    for (uint32_t i = 0; i < m; ++i) {
      const float4 a = s_c0[i], b = s_c1[i];
      if (bq_ray_far(a, b, p, d, dd, dt)) continue;
      V3 ip; float t;
      if (q_ray_comp(p, d, dt, a, b, &ip, &t)) best.offer(ip, t, MGF_HIT_BODY, s_idx[i], 0u);
    }
  }
  if (live) {
    if (mask & MGF_QUERY_TERRAIN) {
      const BatchTerrain M = batch_terrain_of(A.T, (uint32_t)c.world);
      if (M.n_nodes) q_ray_terrain(M, p, d, dt, nullptr, best);
    }
    const size_t pix = (size_t)it.y + (size_t)iy * (uint32_t)c.width + ix;
    if (A.depth) A.depth[pix] = best.have ? best.t : dt;
    if (A.out) q_ray_store(A.out + 7 * pix, best);
    if (A.parts) {
      float* o = A.parts + 7 * pix;
      o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = d.x; o[4] = d.y; o[5] = d.z; o[6] = dt;
    }
    if (A.world) A.world[pix] = c.world;
  }
}

// the depth of pixel i from its final record: the hit's t, or the particle's dt where nothing was hit
__global__ __launch_bounds__(kBatchBlock) void k_batch_camera_depth(const int32_t* out, const float* parts, uint32_t n, float* depth) {
  const uint32_t i = blockIdx.x * kBatchBlock + threadIdx.x;
  if (i >= n) return;
  depth[i] = out[7 * (size_t)i] == MGF_HIT_NONE ? parts[7 * (size_t)i + 6] : u2f((uint32_t)out[7 * (size_t)i + 6]);
}

}  // namespace mgf
