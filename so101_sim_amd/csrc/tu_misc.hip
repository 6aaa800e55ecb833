// Translation unit: physics-only stepping, the parity-test stage dump, contact sensing, proximity sensing, reward, episode bookkeeping (Newton), the cameras (depth / segmentation and colour), Cartesian tool control
// of both engines (the chain kernels for 6 columns - SO100 - and 8 - the general-tree engine, both builds).
#include "so101_kernels.hpp"
#include "so101_contacts.hpp"
#include "so101_proximity.hpp"
#include "so101_camera.hpp"
#include "so101_shade.hpp"
#include "so101_tool_chain.hpp"
#include "so101_launch.hpp"

__global__ void __launch_bounds__(64) k_begin(const DevModel* m, StepParams P, DevBuffers B, unsigned char* need_reset) {
  int e = blockIdx.x, lane = wave_lane(), N = P.n_envs;
  if (lane < NARM) {
    float q = B.qpos[(size_t)lane * N + e];
    for (int r = 0; r < 5; r++) B.ring[((size_t)r * NARM + lane) * N + e] = q;
    B.ctrl[(size_t)lane * N + e] = m->home_ctrl[lane] + P.action_offset[lane];
  }
  if (lane == 0) { B.step_count[e] = 0; B.ep_return[e] = 0.f; need_reset[e] = 0; }
  if (B.ps_ring && lane < PS_DIM) {           // physics_state delay line: padded with the state the episode starts from
    float v = lane < NQ ? B.qpos[(size_t)lane * N + e] : B.qvel[(size_t)(lane - NQ) * N + e];
    for (int r = 0; r < PS_DELAY; r++) B.ps_ring[((size_t)r * PS_DIM + lane) * N + e] = v;
    B.ps_out[(size_t)e * PS_DIM + lane] = v; B.ps_delayed[(size_t)e * PS_DIM + lane] = v;
  }
}

__global__ void __launch_bounds__(64) k_reward(const DevModel* m, StepParams P, DevBuffers B, float* reward) {
  __shared__ EnvLDS L;
  int e = blockIdx.x;
  load_state(L, B, e, P.n_envs);
  kinematics(m, L);
  float r = task_reward(m, L);
  if (wave_lane() == 0) reward[e] = r;
}

namespace so101 {
void launch_physics(int solver, int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B,
                    int nsub, int freeze, int* diag) {
  if (solver == 0) { launch_physics_pgs(n_envs, st, m, P, B, nsub, freeze, diag); return; }
  hipLaunchKernelGGL(k_physics<1>, dim3(n_envs), dim3(64), 0, st, m, P, B, nsub, freeze, diag);
}
void launch_debug_forward(int solver, int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, float* out) {
  if (solver == 0) { launch_debug_forward_pgs(n_envs, st, m, P, B, out); return; }
  hipLaunchKernelGGL(k_debug_forward<1>, dim3(n_envs), dim3(64), 0, st, m, P, B, out);
}
void launch_contacts(int solver, int n, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const int* env_index, int forces,
                     const TouchPairsT<4>& T, const ContactOut& O) {
  if (solver == 0) { launch_contacts_pgs(n, st, m, P, B, env_index, forces, T, O); return; }
  hipLaunchKernelGGL(k_contacts<1>, dim3((unsigned int)n), dim3(64), 0, st, m, P, B, env_index, forces, T, O);
}
void launch_proximity(int n, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const int* env_index, const float* q,
                      const TouchPairsT<4>& T, float max_dist, const ProxOut& O) {
  hipLaunchKernelGGL(k_proximity, dim3((unsigned int)n * (unsigned int)T.npair), dim3(64), 0, st, m, P, B, env_index, q, T, max_dist, O);
}
void launch_begin(int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, unsigned char* need_reset) {
  hipLaunchKernelGGL(k_begin, dim3(n_envs), dim3(64), 0, st, m, P, B, need_reset);
}
void launch_reward(int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, float* reward) {
  hipLaunchKernelGGL(k_reward, dim3(n_envs), dim3(64), 0, st, m, P, B, reward);
}
void launch_render_image(int n_render, hipStream_t st, const DevModel* m, const float* frames, const float* camframes, const float* planes, const int* plane_adr,
                         int ncam, int height, int width, float* depth, int* seg) {
  unsigned int tiles = (unsigned int)((height + 7) / 8) * (unsigned int)((width + 7) / 8);
  hipLaunchKernelGGL(k_render, dim3((unsigned int)n_render * (unsigned int)ncam * tiles), dim3(64), 0, st, m, frames, camframes, planes, plane_adr, ncam, height, width,
                     depth, seg);
}
void launch_shade_image(int n_render, hipStream_t st, const DevModel* m, const float* frames, const float* camframes, const float* planes, const int* plane_adr,
                        int ncam, int height, int width, const float* depth, const int* seg, const float* geom_rgb, int rgb_per_env, const int* env_index,
                        const ShadeParams& S, unsigned char* rgb, float* normal) {
  unsigned int tiles = (unsigned int)((height + 7) / 8) * (unsigned int)((width + 7) / 8);
  hipLaunchKernelGGL(k_shade, dim3((unsigned int)n_render * (unsigned int)ncam * tiles), dim3(64), 0, st, m, frames, camframes, planes, plane_adr, ncam, height, width,
                     depth, seg, geom_rgb, rgb_per_env, env_index, S, rgb, normal);
}
void launch_render(int n_render, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const int* env_index, const RenderCams& cams,
                   int ncam, int height, int width, const float* planes, const int* plane_adr, float* frames, float* camframes,
                   float* depth, int* seg) {
  hipLaunchKernelGGL(k_render_frames, dim3(n_render), dim3(64), 0, st, m, P, B, env_index, cams, ncam, frames, camframes);
  launch_render_image(n_render, st, m, frames, camframes, planes, plane_adr, ncam, height, width, depth, seg);
}
template <int NC>
void launch_tool_pose(int n, hipStream_t st, const ToolChain<NC>& T, const float* q, const float* qpos, int n_envs, const int* env_index,
                      float* pos, float* mat, float* jac) {
  hipLaunchKernelGGL(k_tool_pose<NC>, dim3((unsigned int)((n + WAVE - 1) / WAVE)), dim3(64), 0, st, T, q, qpos, n_envs, env_index, n, pos, mat, jac);
}
template <int NC>
void launch_tool_ik(int n, hipStream_t st, const ToolChain<NC>& T, const IkSettings<NC>& C, const float* target_pos, const float* target_mat,
                    const float* q_init, const float* qpos, int n_envs, const int* env_index, float* q_out, float* residual, int* info) {
  hipLaunchKernelGGL(k_tool_ik<NC>, dim3((unsigned int)((n + WAVE - 1) / WAVE)), dim3(64), 0, st, T, C, target_pos, target_mat, q_init, qpos, n_envs, env_index, n,
                     q_out, residual, info);
}
template void launch_tool_pose<6>(int, hipStream_t, const ToolChain<6>&, const float*, const float*, int, const int*, float*, float*, float*);
template void launch_tool_pose<8>(int, hipStream_t, const ToolChain<8>&, const float*, const float*, int, const int*, float*, float*, float*);
template void launch_tool_ik<6>(int, hipStream_t, const ToolChain<6>&, const IkSettings<6>&, const float*, const float*, const float*, const float*, int, const int*,
                                float*, float*, int*);
template void launch_tool_ik<8>(int, hipStream_t, const ToolChain<8>&, const IkSettings<8>&, const float*, const float*, const float*, const float*, int, const int*,
                                float*, float*, int*);
}  // namespace so101
