// Depth and segmentation cameras of the SO100 engine (so101_render of include/so101.h): batched ray casting against the collision geometry.
//
// Two kernels.  k_render_frames (below; one wavefront per rendered env) runs the step's own kinematics() on the bound qpos and publishes, per geom,
// the world frame load_geom_at() gives the collision code plus the bounding sphere (geom_center, geom_rbound), and the world frames of the
// cameras.  k_render (so101_raycast.hpp, where the definition of a pixel is written down) consumes ONLY those frames and the geom tables -
// nothing of EnvLDS; the general-tree engine feeds the same kernel from k_tree_render_frames (tu_tree.hip).
#pragma once
#include "so101_env.hpp"
#include "so101_raycast.hpp"

// ---------------------------------------------------------------------------------------------------- frames
// env_index: device array of n_render env indices or NULL (block i renders env i).  An index outside [0, n_envs) gives frames nothing can
// hit (every pixel of that image is a miss) instead of an out-of-bounds read.
__global__ void __launch_bounds__(64) k_render_frames(const DevModel* m, StepParams P, DevBuffers B, const int* env_index, RenderCams cams, int ncam,
                                                      float* frames, float* camframes) {
  __shared__ EnvLDS L;
  const int i = blockIdx.x, lane = wave_lane(), N = P.n_envs;
  int e = env_index ? env_index[i] : i;
  e = wave_uniform_i(e);
  const bool ok = e >= 0 && e < N;
  load_state(L, B, ok ? e : 0, N);
  kinematics(m, L);
  const int ngeom = m->ngeom;
  for (int g = lane; g < ngeom; g += WAVE) {
    int d = m->geom_dyn[g];
    GeomW G;
    load_geom_at<G16>(m, g, L.xpos[d < 0 ? 0 : d], L.xmat[d < 0 ? 0 : d], G);
    float* f = frames + ((size_t)i * ngeom + g) * RENDER_FRAME;
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = G.R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) { f[9 + k] = G.p[k]; f[12 + k] = G.c[k]; }
    f[15] = ok ? m->geom_rbound[g] : -1.f;
  }
  // cameras: composed with their body's pose on wave-uniform values (constant indices into the kernel argument), lane 0 publishes
#pragma unroll
  for (int k = 0; k < RENDER_MAXCAM; k++) {
    if (k >= ncam) break;
    const int b = cams.cam[k].body;
    float X[9], P0[3], cp[3], cm[9];
#pragma unroll
    for (int j = 0; j < 9; j++) { X[j] = b < 0 ? (j % 4 == 0 ? 1.f : 0.f) : L.xmat[b < 0 ? 0 : b][j]; cm[j] = cams.cam[k].mat[j]; }
#pragma unroll
    for (int j = 0; j < 3; j++) { P0[j] = b < 0 ? 0.f : L.xpos[b < 0 ? 0 : b][j]; cp[j] = cams.cam[k].pos[j]; }
    float t[3], M[9]; matvec3(t, X, cp); matmul3(M, X, cm);
    if (lane == 0) {
      float* f = camframes + ((size_t)i * ncam + k) * RENDER_CAMFRAME;
#pragma unroll
      for (int j = 0; j < 3; j++) f[j] = P0[j] + t[j];
#pragma unroll
      for (int j = 0; j < 9; j++) f[3 + j] = M[j];
      f[12] = cams.cam[k].scale;
    }
  }
}
