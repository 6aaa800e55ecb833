// Colour cameras (so101_render_color / so101_tree_render_color of include/so101.h): surface normals and Lambert-shaded flat colours of the
// COLLISION geometry k_render (so101_raycast.hpp) casts its rays against.  k_shade runs after k_render on the same stream (one wavefront per
// 8 x 8 pixel tile of one (env, camera), lane = pixel, the grid of k_render) and consumes what k_render wrote - depth and seg of the tile - and
// what k_render consumed: the published RENDER_FRAME / RENDER_CAMFRAME records, the geom tables, the hull planes; and the colours.  Nothing of
// an engine's working set, so the library holds ONE copy: tu_misc.hip compiles it, launch_shade_image (so101_launch.hpp) is what both engines call.
//
// Definition of a pixel (the contract the tests' fp64 reference, tests/shade_ref.py, implements as well):
//   ray, hit, depth, seg   those of k_render; this kernel never changes them
//   normal  world frame, unit: the outward normal of the feature through which the ray enters the hit geom, in the geom frame, rotated by the
//           geom's world matrix.  With x = o_l + t d_l the hit point in the geom frame (t = depth):
//             plane     +z
//             sphere    x / |x|
//             capsule   x minus its projection onto the axis segment |z| <= size[1], normalised (the side and both end balls)
//             cylinder  the side (radial direction of x) if the side's entry parameter is >= the slab's, else the cap (0, 0, -sign(d_l.z))
//             box       the axis whose slab entry parameter is largest, x before y before z at equal values: -sign(d_l[axis]) along it
//             mesh      the hull plane with the largest t = -num / den among those with den < 0, the first in plane order at equal t: its n
//           no hit: 0.  A hit normal faces the camera (n . d < 0).
//   rgb     hit on geom g: v_k = clamp(C_g[k] (A[k] + sum_l D_l[k] max(0, -n . u_l)), 0, 1), byte (uint8)(255 v_k + 0.5); C_g the geom's colour,
//           A the ambient term, u_l the unit world direction light l travels - for a headlight the camera's viewing direction (minus the z
//           column of the camera's world matrix).  No hit: the background colour, converted the same way.
//   bits    a pixel depends on the env's qpos, the camera, (r, c, H, W), that env's colours and the shading only: the loop below runs over the
//           distinct geoms the tile hit, every lane's arithmetic is its own and a lane keeps only what it computed for its own geom.
// This is not MuJoCo's renderer: no textures, shadows, specular term, visual-only meshes or positional lights.
#pragma once
#include "so101_raycast.hpp"

DEV float shade_sign(float v) { return v < 0.f ? -1.f : 1.f; }
DEV unsigned char shade_byte(float v) { return (unsigned char)(255.f * fminf(fmaxf(v, 0.f), 1.f) + 0.5f); }

// grid: that of k_render.  depth / seg: what k_render wrote for the same call (both needed).  geom_rgb [ngeom][3], or [n_envs][ngeom][3] with
// rgb_per_env (entry i reads the row of env env_index[i], i without env_index; an env outside the batch hits nothing and reads nothing).
// rgb [n_render][ncam][H][W][3] uint8, normal the same in float: either may be NULL.
__global__ void __launch_bounds__(64) k_shade(const DevModel* m, const float* frames, const float* camframes, const float* planes, const int* plane_adr,
                                              int ncam, int H, int W, const float* depth, const int* seg, const float* geom_rgb, int rgb_per_env,
                                              const int* env_index, ShadeParams S, unsigned char* rgb, float* normal) {
  const int lane = wave_lane();
  const unsigned int tx = (unsigned int)(W + 7) >> 3, ty = (unsigned int)(H + 7) >> 3;
  unsigned int b = blockIdx.x;
  const unsigned int bx = b % tx; b /= tx;
  const unsigned int by = b % ty; b /= ty;
  const unsigned int cam = b % (unsigned int)ncam, i = b / (unsigned int)ncam;
  const int r = (int)(by * 8u) + (lane >> 3), c = (int)(bx * 8u) + (lane & 7);
  const bool inside = r < H && c < W;
  const size_t px = (((size_t)i * ncam + cam) * H + (inside ? r : 0)) * W + (inside ? c : 0);
  // ray in the world: k_render's, statement for statement
  const float* cf = camframes + ((size_t)i * ncam + cam) * RENDER_CAMFRAME;
  float o[3], d[3], view[3];
  {
    const float s = ldc(cf + 12);
    float dc[3] = {((float)c + 0.5f - 0.5f * (float)W) * s, -((float)r + 0.5f - 0.5f * (float)H) * s, -1.f};
    float M[9];
#pragma unroll
    for (int k = 0; k < 9; k++) M[k] = ldc(cf + 3 + k);
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = ldc(cf + k);
    matvec3(d, M, dc);
    view[0] = -M[2]; view[1] = -M[5]; view[2] = -M[8];
  }
  const int mine = inside ? seg[px] : -1;
  const float t = inside ? depth[px] : RENDER_INF;
  const int ngeom = ldc(&m->ngeom);
  const int* gtype = ldc(&m->geom_type);
  const float* gsize = ldc(&m->geom_size);
  float n[3] = {0.f, 0.f, 0.f};
  bool pending = mine >= 0 && mine < ngeom;
  // wave-uniform loop over the distinct geoms of the tile: the geom of the first pending lane, for every lane that hit it
  for (unsigned long long todo = wave_ballot(pending); todo != 0ull; todo = wave_ballot(pending)) {
    const int g = wave_get_i(mine, (int)__builtin_ctzll(todo));
    const float* f = frames + ((size_t)i * ngeom + g) * RENDER_FRAME;
    float R[9], p[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = ldc(f + k);
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = ldc(f + 9 + k);
    const int type = ldc(gtype + g);
    float ol[3], dl[3];
    {
      float w[3] = {o[0] - p[0], o[1] - p[1], o[2] - p[2]};
      matTvec3(ol, R, w); matTvec3(dl, R, d);
    }
    const float s0 = ldc(gsize + 3 * g), s1 = ldc(gsize + 3 * g + 1), s2 = ldc(gsize + 3 * g + 2);
    const float x[3] = {ol[0] + t * dl[0], ol[1] + t * dl[1], ol[2] + t * dl[2]};
    float nl[3] = {0.f, 0.f, 1.f};          // (plane)
    if (type == G_SPHERE) {
      nl[0] = x[0]; nl[1] = x[1]; nl[2] = x[2];
    } else if (type == G_CAPSULE) {
      nl[0] = x[0]; nl[1] = x[1]; nl[2] = x[2] - fminf(fmaxf(x[2], -s1), s1);
    } else if (type == G_CYLINDER) {
      float a0, a1, z0, z1;
      ray_round(ol, dl, 0.f, s0, 2, a0, a1);
      ray_slab(ol[2], dl[2], s1, z0, z1);
      const bool side = a0 >= z0;
      nl[0] = side ? x[0] : 0.f; nl[1] = side ? x[1] : 0.f; nl[2] = side ? 0.f : -shade_sign(dl[2]);
    } else if (type == G_BOX) {
      float x0, x1, y0, y1, z0, z1;
      ray_slab(ol[0], dl[0], s0, x0, x1); ray_slab(ol[1], dl[1], s1, y0, y1); ray_slab(ol[2], dl[2], s2, z0, z1);
      int axis = 0;
      float e = x0;
      if (y0 > e) { e = y0; axis = 1; }
      if (z0 > e) { e = z0; axis = 2; }
      nl[0] = axis == 0 ? -shade_sign(dl[0]) : 0.f; nl[1] = axis == 1 ? -shade_sign(dl[1]) : 0.f; nl[2] = axis == 2 ? -shade_sign(dl[2]) : 0.f;
    } else if (type == G_MESH) {
      // the planes stream through at wave-uniform addresses, as in k_render; strict >: the first plane keeps an equal t
      const int k0 = ldc(plane_adr + g), k1 = ldc(plane_adr + g + 1);
      float e = -RENDER_INF;
      for (int j = k0; j < k1; j++) {
        const float* pl = planes + 4 * (size_t)j;
        float nx = ldc(pl), ny = ldc(pl + 1), nz = ldc(pl + 2), nd = ldc(pl + 3);
        float den = nx * dl[0] + ny * dl[1] + nz * dl[2];
        float num = nx * ol[0] + ny * ol[1] + nz * ol[2] + nd;
        float tt = -num / den;
        if (den < 0.f && tt > e) { e = tt; nl[0] = nx; nl[1] = ny; nl[2] = nz; }
      }
    }
    if (pending && mine == g) {
      float nw[3];
      matvec3(nw, R, nl);
      const float len = sqrtf(dot3(nw, nw));
      const float inv = len > 0.f ? 1.f / len : 0.f;
      n[0] = nw[0] * inv; n[1] = nw[1] * inv; n[2] = nw[2] * inv;
      pending = false;
    }
  }
  if (!inside) return;
  if (normal) { normal[3 * px] = n[0]; normal[3 * px + 1] = n[1]; normal[3 * px + 2] = n[2]; }
  if (rgb) {
    float v[3] = {S.background[0], S.background[1], S.background[2]};
    if (mine >= 0 && mine < ngeom) {
      float li[3] = {S.ambient[0], S.ambient[1], S.ambient[2]};
#pragma unroll
      for (int l = 0; l < SHADE_MAXLIGHT; l++) {
        if (l < S.nlight) {
          const bool head = S.headlight[l] != 0;
          const float ux = head ? view[0] : S.dir[l][0], uy = head ? view[1] : S.dir[l][1], uz = head ? view[2] : S.dir[l][2];
          const float w = fmaxf(0.f, -(n[0] * ux + n[1] * uy + n[2] * uz));
          li[0] += S.diffuse[l][0] * w; li[1] += S.diffuse[l][1] * w; li[2] += S.diffuse[l][2] * w;
        }
      }
      size_t row = 0;
      if (rgb_per_env) row = (size_t)(env_index ? env_index[i] : (int)i) * (size_t)ngeom;
      const float* col = geom_rgb + 3 * (row + (size_t)mine);
      v[0] = col[0] * li[0]; v[1] = col[1] * li[1]; v[2] = col[2] * li[2];
    }
    rgb[3 * px] = shade_byte(v[0]); rgb[3 * px + 1] = shade_byte(v[1]); rgb[3 * px + 2] = shade_byte(v[2]);
  }
}
