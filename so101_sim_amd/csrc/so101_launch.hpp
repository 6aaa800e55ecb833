// Host-side launchers, one per kernel.  Each is defined in the translation unit that holds the kernel (tu_*.hip):
// without relocatable device code a kernel can only be launched from the file it is compiled in, and splitting the
// kernels over several files lets the library build in parallel.  `solver`: 1 = Newton, 0 = PGS (include/so101.h).
#pragma once
#include <hip/hip_runtime.h>
#include "so101_model.hpp"

template <int NC> struct ToolChain;          // so101_tool_chain.hpp
template <int NC> struct IkSettings;
template <int NW> struct TouchPairsT;        // so101_contact_report.hpp

namespace so101 {

struct StepIO {            // per-call arrays of so101_step (device pointers)
  const float* action; float* obs; float* reward; float* discount; unsigned char* step_type;
};

// fused kernels -------------------------------------------------------------------------------------------------
void launch_reset(int solver, int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B,
                  const PrepBuffers& C, const EventBuffers& E, const unsigned char* mask, unsigned char* need_reset, int* diag);
void launch_settle(int solver, int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const EventBuffers& E, int* diag);
void launch_settle_table(int solver, int n_envs, int first, int count, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B,
                         float* qpos, float* qvel, float* warm, int* flags);
void launch_prepare(int waves, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const PrepBuffers& C);   // Newton
void launch_step(int solver, int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B,
                 const PrepBuffers& C, const EventBuffers& E, const StepIO& io, unsigned char* need_reset, int* diag);
void launch_physics(int solver, int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B,
                    int nsub, int freeze, int* diag);
void launch_debug_forward(int solver, int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, float* out);
// contact sensing (so101_contacts.hpp): one wavefront per reported env, n of them; env_index NULL = envs 0 .. n - 1
void launch_contacts(int solver, int n, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const int* env_index, int forces,
                     const TouchPairsT<4>& T, const ContactOut& O);
// proximity sensing (so101_proximity.hpp): one wavefront per (entry, pair), n * T.npair of them; q NULL = the bound arm angles
void launch_proximity(int n, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const int* env_index, const float* q,
                      const TouchPairsT<4>& T, float max_dist, const ProxOut& O);
void launch_begin(int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, unsigned char* need_reset);
void launch_reward(int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, float* reward);

// depth / segmentation cameras.  launch_render_image: k_render (so101_raycast.hpp), one wavefront per 8 x 8 tile of every (env, camera) image, from
// frames an engine's frames kernel published on the same stream - the ONE copy of k_render in the library, called by both engines (the
// general-tree engine after its k_tree_render_frames, tu_tree.hip).  launch_render: the SO100 frames kernel (so101_camera.hpp), then the image.
void launch_render_image(int n_render, hipStream_t st, const DevModel* m, const float* frames, const float* camframes, const float* planes, const int* plane_adr,
                         int ncam, int height, int width, float* depth, int* seg);
// colour cameras.  launch_shade_image: k_shade (so101_shade.hpp) on the grid of k_render, after it on the same stream, from the depth / seg it wrote -
// like k_render ONE copy in the library, called by both engines.  rgb / normal: either may be NULL.
void launch_shade_image(int n_render, hipStream_t st, const DevModel* m, const float* frames, const float* camframes, const float* planes, const int* plane_adr,
                        int ncam, int height, int width, const float* depth, const int* seg, const float* geom_rgb, int rgb_per_env, const int* env_index,
                        const ShadeParams& S, unsigned char* rgb, float* normal);
void launch_render(int n_render, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const int* env_index, const RenderCams& cams,
                   int ncam, int height, int width, const float* planes, const int* plane_adr, float* frames, float* camframes,
                   float* depth, int* seg);

// Cartesian tool control (so101_tool_chain.hpp): lane = entry, one wavefront per 64 entries; NC = 6 (SO100) and NC = 8 (the general-tree engine, both
// builds) are instantiated.  q / q_init: [n][T.nio] or NULL = the bound qpos of env env_index[i] (NULL: i)
template <int NC>
void launch_tool_pose(int n, hipStream_t st, const ToolChain<NC>& T, const float* q, const float* qpos, int n_envs, const int* env_index,
                      float* pos, float* mat, float* jac);
template <int NC>
void launch_tool_ik(int n, hipStream_t st, const ToolChain<NC>& T, const IkSettings<NC>& C, const float* target_pos, const float* target_mat,
                    const float* q_init, const float* qpos, int n_envs, const int* env_index, float* q_out, float* residual, int* info);

// pipelined step (Newton) -----------------------------------------------------------------------------------------
void launch_order(hipStream_t st, const unsigned int* cost, int* order, unsigned char* cls, int n_envs, int deal = 1);   // deal: equal slices the sorted envs are dealt to (1 = plain sorted order)
void launch_pipe_begin(int n_group, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const PrepBuffers& C,
                       const EventBuffers& E, const PipeBuffers& W, const StepIO& io, unsigned char* need_reset, int* diag, int e0,
                       const ChainParams* chain = nullptr);
void launch_narrow(int waves, hipStream_t st, const DevModel* m, int n_envs, const PipeBuffers& W, int substep);
void launch_pipe_solve(int n_group, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const EventBuffers& E,
                       const PipeBuffers& W, int substep, int last, const StepIO& io, unsigned char* need_reset, int* diag, int e0);

// merged launches (pipeline = 3): solve of substep s + narrowphase chunks of substep s + 1 in one launch per chain
void launch_pipe_merged(int n_group, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const EventBuffers& E,
                        const PipeBuffers& W, int substep, int last, int launch, const StepIO& io, unsigned char* need_reset, int* diag, int e0);

// per-env chained step (so101_chain.hpp): k_order + k_pipe_begin + ONE persistent launch
void launch_chain(int waves, hipStream_t st, const ChainParams* params /* device memory */);

// the PGS instantiations live in their own files
void launch_reset_pgs(int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const PrepBuffers& C,
                      const EventBuffers& E, const unsigned char* mask, unsigned char* need_reset, int* diag);
void launch_settle_pgs(int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const EventBuffers& E, int* diag);
void launch_settle_table_pgs(int n_envs, int first, int count, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B,
                             float* qpos, float* qvel, float* warm, int* flags);
void launch_step_pgs(int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const PrepBuffers& C,
                     const EventBuffers& E, const StepIO& io, unsigned char* need_reset, int* diag);
void launch_physics_pgs(int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, int nsub, int freeze, int* diag);
void launch_debug_forward_pgs(int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, float* out);
void launch_contacts_pgs(int n, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const int* env_index, int forces,
                         const TouchPairsT<4>& T, const ContactOut& O);

}  // namespace so101
