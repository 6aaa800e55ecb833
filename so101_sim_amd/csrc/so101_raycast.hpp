// Ray casting of the depth and segmentation cameras (so101_render / so101_tree_render of include/so101.h): the image kernel and the ray
// against MuJoCo's primitive shapes.  k_render (one wavefront per 8 x 8 pixel tile of one (env, camera), lane = pixel) consumes ONLY the world
// frames a frames kernel published (RENDER_FRAME / RENDER_CAMFRAME records, so101_model.hpp) and the geom tables of a DevModel - nothing of an
// engine's per-env working set - so each engine feeds it from a frames kernel of its own: k_render_frames (so101_camera.hpp, SO100) and
// k_tree_render_frames (tu_tree.hip, the general-tree engine).  The library holds ONE copy of k_render: tu_misc.hip compiles it and defines
// the launcher (launch_render_image, so101_launch.hpp) both engines call.
//
// Definition of a pixel (the contract the tests' fp64 reference implements as well):
//   ray     pixel (r, c) of an H x W image: camera-frame direction ((c + 0.5 - W/2) s, -(r + 0.5 - H/2) s, -1), s = 2 tan(fovy / 2) / H, from
//           the camera position.  The direction is not normalised: the ray parameter t IS the distance along the optical axis.
//   depth   t of the nearest hit, +inf without one; seg the geom index, -1 without one; equal t: the lower geom index.
//   geoms   MuJoCo's shapes and sizes; a mesh is the convex polytope of its facet planes (so101_set_hull_planes); a plane is hit from its
//           front side only and clipped to +-size where size > 0; a hit needs t > 0; a geom whose interior holds the ray origin is invisible
//           (for the convex solids: the line meets the solid in [t_enter, t_exit], a hit is t_enter <= t_exit and t_enter > 0).
//   bits    a pixel depends on the env's qpos, the camera and (r, c, H, W) only: the loop over geoms is wave-uniform, every lane's arithmetic
//           is its own, and the early exits below only ever skip work whose result the lane would discard.
#pragma once
#include "so101_geom.hpp"

#define RENDER_PLANE_CHUNK 8     // hull planes between two "can any lane still improve" ballots

// ---------------------------------------------------------------------------------------------------- ray against the primitives
#define RENDER_INF __builtin_inff()

// the line o + t d against the slab |x| <= h of one coordinate: [t0, t1], empty (t0 > t1) when it runs beside the slab
DEV void ray_slab(float o, float d, float h, float& t0, float& t1) {
  if (d != 0.f) {
    float a = (-h - o) / d, b = (h - o) / d;
    t0 = fminf(a, b); t1 = fmaxf(a, b);
  } else {
    bool in = fabsf(o) <= h;
    t0 = in ? -RENDER_INF : RENDER_INF; t1 = in ? RENDER_INF : -RENDER_INF;
  }
}
// the line against the ball |x - (0, 0, cz)| <= r (ndim 3) or the infinite cylinder x^2 + y^2 <= r^2 (ndim 2): through the point of closest
// approach, so that a small shape far away loses no digits to b^2 - a c
DEV void ray_round(const float* o, const float* d, float cz, float r, int ndim, float& t0, float& t1) {
  float oz = ndim == 3 ? o[2] - cz : 0.f, dz = ndim == 3 ? d[2] : 0.f;
  float a = d[0] * d[0] + d[1] * d[1] + dz * dz;
  float b = o[0] * d[0] + o[1] * d[1] + oz * dz;
  if (a > 0.f) {
    float tc = -b / a;
    float wx = o[0] + tc * d[0], wy = o[1] + tc * d[1], wz = oz + tc * dz;
    float q = r * r - (wx * wx + wy * wy + wz * wz);
    float half = sqrtf(fmaxf(q, 0.f) / a);
    t0 = q >= 0.f ? tc - half : RENDER_INF; t1 = q >= 0.f ? tc + half : -RENDER_INF;
  } else {      // (ndim 2: the ray runs along the axis)
    bool in = o[0] * o[0] + o[1] * o[1] + oz * oz <= r * r;
    t0 = in ? -RENDER_INF : RENDER_INF; t1 = in ? RENDER_INF : -RENDER_INF;
  }
}

// ---------------------------------------------------------------------------------------------------- the image
// grid: n_render * ncam * tiles_y * tiles_x blocks of one wavefront; depth / seg [n_render][ncam][H][W] (either may be NULL)
__global__ void __launch_bounds__(64) k_render(const DevModel* m, const float* frames, const float* camframes, const float* planes, const int* plane_adr,
                                               int ncam, int H, int W, float* depth, int* seg) {
  const int lane = wave_lane();
  const unsigned int tx = (unsigned int)(W + 7) >> 3, ty = (unsigned int)(H + 7) >> 3;
  unsigned int b = blockIdx.x;
  const unsigned int bx = b % tx; b /= tx;
  const unsigned int by = b % ty; b /= ty;
  const unsigned int cam = b % (unsigned int)ncam, i = b / (unsigned int)ncam;
  const int r = (int)(by * 8u) + (lane >> 3), c = (int)(bx * 8u) + (lane & 7);
  const bool inside = r < H && c < W;
  // ray in the world
  const float* cf = camframes + ((size_t)i * ncam + cam) * RENDER_CAMFRAME;
  float o[3], d[3];
  {
    const float s = ldc(cf + 12);
    float dc[3] = {((float)c + 0.5f - 0.5f * (float)W) * s, -((float)r + 0.5f - 0.5f * (float)H) * s, -1.f};
    float M[9];
#pragma unroll
    for (int k = 0; k < 9; k++) M[k] = ldc(cf + 3 + k);
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = ldc(cf + k);
    matvec3(d, M, dc);
  }
  const float dd = dot3(d, d), dlen = sqrtf(dd);
  float best = RENDER_INF;
  int hit = -1;
  const int ngeom = ldc(&m->ngeom);
  const int* gtype = ldc(&m->geom_type);
  const float* gsize = ldc(&m->geom_size);
  for (int g = 0; g < ngeom; g++) {
    const float* f = frames + ((size_t)i * ngeom + g) * RENDER_FRAME;
    float R[9], p[3], ctr[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = ldc(f + k);
#pragma unroll
    for (int k = 0; k < 3; k++) { p[k] = ldc(f + 9 + k); ctr[k] = ldc(f + 12 + k); }
    const float rb = ldc(f + 15);
    const int type = ldc(gtype + g);
    if (rb < 0.f) continue;
    if (type != G_PLANE) {
      // bounding sphere, widened beyond any rounding of the test itself (it only ever decides to SKIP work): no lane can hit the geom, or
      // none can hit it nearer than what it has
      float rr = rb * 1.0001f + 1e-6f;
      float oc[3] = {ctr[0] - o[0], ctr[1] - o[1], ctr[2] - o[2]};
      float bq = dot3(oc, d), l2 = dot3(oc, oc);
      bool may = l2 * dd - bq * bq <= rr * rr * dd * 1.0001f + 1e-6f * l2 * dd && (bq > 0.f || l2 <= rr * rr);
      may = may && (bq - rr * dlen) <= best * dd * 1.0001f;
      if (wave_ballot(inside && may) == 0ull) continue;
    }
    // the ray in the geom's frame (t is unchanged: a rigid map, no normalisation)
    float ol[3], dl[3];
    {
      float w[3] = {o[0] - p[0], o[1] - p[1], o[2] - p[2]};
      matTvec3(ol, R, w); matTvec3(dl, R, d);
    }
    const float s0 = ldc(gsize + 3 * g), s1 = ldc(gsize + 3 * g + 1), s2 = ldc(gsize + 3 * g + 2);
    float t0 = RENDER_INF, t1 = -RENDER_INF;      // [t_enter, t_exit] of the line in the solid
    if (type == G_PLANE) {
      // front side only: from z > 0 heading down; clipped to +-size where size > 0.  t1 = inf: a plane has no far side to compare with
      float t = -ol[2] / dl[2];
      float x = ol[0] + t * dl[0], y = ol[1] + t * dl[1];
      bool on = dl[2] < 0.f && ol[2] > 0.f && (s0 <= 0.f || fabsf(x) <= s0) && (s1 <= 0.f || fabsf(y) <= s1);
      t0 = on ? t : RENDER_INF; t1 = on ? RENDER_INF : -RENDER_INF;
    } else if (type == G_SPHERE) {
      ray_round(ol, dl, 0.f, s0, 3, t0, t1);
    } else if (type == G_CAPSULE || type == G_CYLINDER) {
      float a0, a1, z0, z1;
      ray_round(ol, dl, 0.f, s0, 2, a0, a1);
      ray_slab(ol[2], dl[2], s1, z0, z1);
      t0 = fmaxf(a0, z0); t1 = fminf(a1, z1);
      if (type == G_CAPSULE) {
        // the union of the side and the two end balls is convex: the line meets it in [min of the entries, max of the exits]
        bool any = t0 <= t1;
        float e0 = any ? t0 : RENDER_INF, e1 = any ? t1 : -RENDER_INF;
#pragma unroll
        for (int k = 0; k < 2; k++) {
          float c0, c1;
          ray_round(ol, dl, k ? -s1 : s1, s0, 3, c0, c1);
          bool h = c0 <= c1;
          e0 = h ? fminf(e0, c0) : e0; e1 = h ? fmaxf(e1, c1) : e1;
        }
        t0 = e0; t1 = e1;
      }
    } else if (type == G_BOX) {
      float x0, x1, y0, y1, z0, z1;
      ray_slab(ol[0], dl[0], s0, x0, x1); ray_slab(ol[1], dl[1], s1, y0, y1); ray_slab(ol[2], dl[2], s2, z0, z1);
      t0 = fmaxf(fmaxf(x0, y0), z0); t1 = fminf(fminf(x1, y1), z1);
    } else {
      // convex hull: the planes n . x + d <= 0 stream through at wave-uniform addresses; t_enter = max over the planes the ray enters
      // through, t_exit = min over those it leaves through.  Left as soon as no lane can still improve on what it has.
      const int k0 = ldc(plane_adr + g), k1 = ldc(plane_adr + g + 1);
      t0 = -RENDER_INF; t1 = RENDER_INF;
      for (int k = k0; k < k1; k += RENDER_PLANE_CHUNK) {
        const int ke = k + RENDER_PLANE_CHUNK < k1 ? k + RENDER_PLANE_CHUNK : k1;
        for (int j = k; j < ke; j++) {
          const float* pl = planes + 4 * (size_t)j;
          float nx = ldc(pl), ny = ldc(pl + 1), nz = ldc(pl + 2), nd = ldc(pl + 3);
          float den = nx * dl[0] + ny * dl[1] + nz * dl[2];
          float num = nx * ol[0] + ny * ol[1] + nz * ol[2] + nd;      // signed distance of the origin: > 0 outside this plane
          float t = -num / den;
          t0 = den < 0.f ? fmaxf(t0, t) : t0;
          t1 = den > 0.f ? fminf(t1, t) : t1;
          if (den == 0.f && num > 0.f) t0 = RENDER_INF;              // parallel to the plane and outside it
        }
        if (wave_ballot(inside && t0 <= t1 && t0 < best) == 0ull) break;
      }
    }
    // strict <: of two geoms at the same t the lower index, seen first, stays
    if (t0 <= t1 && t0 > 0.f && t0 < best) { best = t0; hit = g; }
  }
  if (inside) {
    size_t px = (((size_t)i * ncam + cam) * H + r) * W + c;
    if (depth) depth[px] = best;
    if (seg) seg[px] = hit;
  }
}
