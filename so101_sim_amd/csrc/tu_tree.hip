// General-tree engine: the so101_tree_* entry points of include/so101.h over its device functions (so101_tree.hpp), kernels
// (so101_tree_kernels.hpp) and host code (so101_tree_host.hpp).  Kernels and their launches live in one translation unit (no relocatable device code).
#include <hip/hip_runtime.h>
#include "so101_host.hpp"
#include "so101_launch.hpp"
#include "so101_tree.hpp"

// entry points of this build: so101_tree32_* / so101_tree64_*; the public so101_tree_* of include/so101.h dispatch on the handle
// (csrc/tu_tree_api.hip)
#undef TAPI
#undef TAPI_CAT
#undef TAPI_CAT2
#define TAPI_CAT2(v, name) so101_tree##v##_##name
#define TAPI_CAT(v, name) TAPI_CAT2(v, name)
#define TAPI(name) TAPI_CAT(TREE_VARIANT, name)

#ifndef TREE_SOLVE_OCC
#if TREE_VARIANT == 64
#define TREE_SOLVE_OCC 1     // (LDS allows two envs per CU: registers are free; the Hessian's four accumulator tiles want them)
#else
#define TREE_SOLVE_OCC 2
#endif
#endif

#include "so101_tree_kernels.hpp"
#include "so101_tree_host.hpp"

namespace TREE_NS {
namespace {
// ---- cameras and colour cameras (k_tree_render_frames, then the library's one k_render through so101::launch_render_image)
// One body for render and render_color (so101_shade.hpp): the depth / seg call is the colour call without shading.  k_tree_render_frames and the
// library's k_render, then - shading asked for - its one k_shade through so101::launch_shade_image.  color: the colour call (outputs in `out`, else
// depth and seg)
int tree_render_call(TreeHandle* s, const std::string& api, bool color, const so101_camera* cams, int ncam, int height, int width, const int32_t* env_index, int n_render,
                            int source, const so101_shading* shading, const float* geom_rgb, int rgb_per_env, const so101_color_out* out, float* depth, int* seg, void* stream) {
  if (!s) return SO101_ERR_ARG;
  RenderCams rc{};
  ShadeParams sp{};
  if (!render_arguments(s, api.c_str(), cams, ncam, height, width, n_render, s->n_envs, env_index != nullptr, color || depth || seg, s->hm.nbody - 1, rc)) return SO101_ERR_ARG;
  if (source != 0 && source != 1) { s->err = api + ": source must be 0 (the bound qpos) or 1 (the delayed physics-state line)"; return SO101_ERR_ARG; }
  if (color && !shade_arguments(s, api.c_str(), shading, geom_rgb, out, sp)) return SO101_ERR_ARG;
  RenderHost& R = s->render;
  if (R.has_meshes() && !R.planes_set) { s->err = api + ": the scene has mesh geoms and no hull planes (call so101_tree_set_hull_planes)"; return SO101_ERR_STATE; }
  if (source == 0 && !s->bound) { s->err = api + " before so101_tree_bind_state"; return SO101_ERR_STATE; }
  if (source == 1 && !s->env.ps_delayed) { s->err = api + ": source 1 needs the physics-state line (so101_tree_bind_physics_state)"; return SO101_ERR_STATE; }
  GUARD_DEVICE(s);
  const bool shade = color && (out->rgb || out->normal);
  if (color) { depth = out->depth; seg = (int*)out->seg; }
  if (!R.reserve(s, (size_t)n_render)) return SO101_ERR_HIP;
  // (the pixel scratch: k_shade reads the depth and seg k_render wrote, so a caller who asks for neither gets them there)
  if (shade && !(depth && seg) && !R.reserve_pixels(s, (size_t)n_render * ncam * height * width)) return SO101_ERR_HIP;
  if (shade && !depth) depth = R.px_depth;
  if (shade && !seg) seg = R.px_seg;
  const float* q = source == 0 ? s->buf.qpos : s->env.ps_delayed;
  const size_t lane_stride = source == 0 ? (size_t)s->n_envs : 1, env_stride = source == 0 ? 1 : (size_t)(s->hm.nq + s->hm.nv);
  hipLaunchKernelGGL(k_tree_render_frames, dim3(n_render), dim3(64), 0, (hipStream_t)stream, s->dm, s->dg, q, lane_stride, env_stride, s->n_envs, (const int*)env_index, rc, ncam,
                     R.frames, R.cams);
  so101::launch_render_image(n_render, (hipStream_t)stream, s->dg, R.frames, R.cams, R.hull_planes, R.plane_adr, ncam, height, width, depth, seg);
  if (!hip_ok(s, hipGetLastError(), "k_render")) return SO101_ERR_HIP;
  if (shade)
    so101::launch_shade_image(n_render, (hipStream_t)stream, s->dg, R.frames, R.cams, R.hull_planes, R.plane_adr, ncam, height, width, depth, seg, geom_rgb, rgb_per_env != 0,
                              (const int*)env_index, sp, out->rgb, out->normal);
  return hip_ok(s, hipGetLastError(), "k_shade") ? SO101_OK : SO101_ERR_HIP;
}
}  // namespace

extern "C" {

int TAPI(create)(const void* blob, size_t bytes, int n_envs, int hip_device, TreeHandle** out) {
  if (!out) return SO101_ERR_ARG;
  *out = nullptr;
  if (!blob || n_envs <= 0) { g_tree_error = "so101_tree_create: bad argument"; return SO101_ERR_ARG; }
  BlobView b;
  if (!b.parse(blob, bytes, g_tree_error)) return SO101_ERR_MODEL;
  TreeHandle* s = new TreeHandle();
  s->n_envs = n_envs; s->device = hip_device;
  int rc = SO101_OK;
  DeviceGuard guard(s);                       // (the caller's current device is restored on every return path)
  if (!guard.ok) rc = SO101_ERR_HIP;
  if (rc == SO101_OK) rc = tree_build(s, b);
  size_t n = (size_t)n_envs;
  if (rc == SO101_OK && !(dev_alloc(s, &s->buf.scratch, n * T_SCRATCH, -1, "hipMalloc(scratch)") && dev_alloc(s, &s->buf.diag, 8 * n, 0, "hipMalloc(diag)") &&
                          dev_alloc(s, &s->env.need_reset, n, 1, "hipMalloc(need_reset)") && dev_alloc(s, &s->env.success_state, n, 0, "hipMalloc(success_state)")))
    rc = SO101_ERR_HIP;
  if (rc != SO101_OK) { g_tree_error = s->err; free_owned(s); delete s; return rc; }
  s->iterations = s->hm.iterations; s->tolerance = s->hm.tolerance;
  *out = s;
  return SO101_OK;
}

void TAPI(destroy)(TreeHandle* s) {
  if (!s) return;
  {
    DeviceGuard guard(s);
    (void)hipDeviceSynchronize();                 // nothing of this handle may still be running on buffers that are about to go
#ifdef TREE_PROF
    {
      unsigned long long h[33] = {};
      (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_tprof), sizeof(h));
      if (h[32]) {
        static const char* nm[32] = {"cost: M x + jar", "cost: blocks", "cost: gradient", "cost: H = M", "cost: H scalar rows", "cost: H contacts", "chol factor", "chol solve",
                                     "ls setup (J search)", "line search", "make_constraints", "newton total", "SMOOTH HALF", "CONSTRAINED HALF", "", "newton loop top (incl. cost)",
                                     "load_state", "kinematics", "crba + factor", "rne", "smooth", "gather_contacts", "euler + check", "store_state", "kinematics (next)", "publish (next broadphase)",
                                     "", "", "", "", "", ""};
        fprintf(stderr, "TREE_PROF k_tree_pipe_solve, %llu env-substeps, mean us each:\n", h[32]);
        for (int k = 0; k < 32; k++) if (nm[k][0]) fprintf(stderr, "  %-30s %8.2f\n", nm[k], (double)h[k] * 1e-2 / (double)h[32]);
      }
    }
#endif
    free_owned(s);
  }
  delete s;
}

const char* TAPI(last_error)(const TreeHandle* s) { return s ? s->err.c_str() : g_tree_error.c_str(); }

int TAPI(dims)(const TreeHandle* s, int* dims /* [16]: nq nv nu nbody ngeom debug_dim max_contacts, then the debug layout (offsets of bias, qacc_smooth, qacc, xpos, M, contacts, forces; row stride of M) and the build (32 / 64) */) {
  if (!s || !dims) return SO101_ERR_ARG;
  dims[0] = s->hm.nq; dims[1] = s->hm.nv; dims[2] = s->hm.nu; dims[3] = s->hm.nbody; dims[4] = s->hm.ngeom; dims[5] = TDBG_DIM; dims[6] = TCON;
  dims[7] = TDBG_BIAS; dims[8] = TDBG_QSM; dims[9] = TDBG_QACC; dims[10] = TDBG_XPOS; dims[11] = TDBG_M; dims[12] = TDBG_CON; dims[13] = TDBG_FORCE; dims[14] = TV; dims[15] = TREE_VARIANT;
  return SO101_OK;
}

int TAPI(last_plan)(const TreeHandle* s, int* out /* [4] */) {
  if (!s || !out) return SO101_ERR_ARG;
  for (int i = 0; i < 4; i++) out[i] = s->plan[i];
  return SO101_OK;
}

int TAPI(bind_state)(TreeHandle* s, float* qpos, float* qvel, float* ctrl, float* warmstart) {
  if (!s || !qpos || !qvel || !ctrl || !warmstart) { if (s) s->err = "so101_tree_bind_state: NULL buffer"; return SO101_ERR_ARG; }
  s->buf.qpos = qpos; s->buf.qvel = qvel; s->buf.ctrl = ctrl; s->buf.warm = warmstart;
  s->bound = true;
  return SO101_OK;
}

int TAPI(configure)(TreeHandle* s, int solver_iterations, float solver_tolerance) {
  if (!s) return SO101_ERR_ARG;
  s->iterations = solver_iterations > 0 ? solver_iterations : s->hm.iterations;
  s->tolerance = solver_tolerance >= 0.f ? solver_tolerance : s->hm.tolerance;
  return SO101_OK;
}

int TAPI(physics)(TreeHandle* s, int n_substeps, void* stream) {
  if (!s || n_substeps < 0) return SO101_ERR_ARG;
  if (!s->bound) { s->err = "so101_tree_physics before so101_tree_bind_state"; return SO101_ERR_STATE; }
  GUARD_DEVICE(s);
  hipLaunchKernelGGL(k_tree_physics, dim3(s->n_envs), dim3(64), 0, (hipStream_t)stream, s->dm, s->dg, s->buf, s->n_envs, n_substeps, s->iterations, s->tolerance);
  return hip_ok(s, hipGetLastError(), "k_tree_physics") ? SO101_OK : SO101_ERR_HIP;
}

int TAPI(debug_forward)(TreeHandle* s, float* out, void* stream) {
  if (!s || !out) return SO101_ERR_ARG;
  if (!s->bound) { s->err = "so101_tree_debug_forward before so101_tree_bind_state"; return SO101_ERR_STATE; }
  GUARD_DEVICE(s);
  static const int phases = getenv("SO101_TREE_PHASES") ? atoi(getenv("SO101_TREE_PHASES")) : 0x7f;      // timing runs only
  hipLaunchKernelGGL(k_tree_forward, dim3(s->n_envs), dim3(64), 0, (hipStream_t)stream, s->dm, s->dg, s->buf, s->n_envs, s->iterations, s->tolerance, out, phases);
  return hip_ok(s, hipGetLastError(), "k_tree_forward") ? SO101_OK : SO101_ERR_HIP;
}

// ---- env layer (hand-over scenes)
int TAPI(obs_dim)(const TreeHandle* s) { return s && s->has_task ? 3 * s->task.npos + 2 * s->task.nvel : 0; }

int TAPI(bind_env)(TreeHandle* s, float* ring_pos, float* ring_vel, float* ep_return, int32_t* step_count, int32_t* episode) {
  if (!s || !ring_pos || !ring_vel || !ep_return || !step_count || !episode) { if (s) s->err = "so101_tree_bind_env: NULL buffer"; return SO101_ERR_ARG; }
  if (!s->has_task) { s->err = "so101_tree_bind_env: the model carries no task (bare-arm blob)"; return SO101_ERR_STATE; }
  s->env.ring_pos = ring_pos; s->env.ring_vel = ring_vel; s->env.ep_return = ep_return; s->env.step_count = step_count; s->env.episode = episode;
  s->env_bound = true;
  return SO101_OK;
}

int TAPI(bind_physics_state)(TreeHandle* s, float* ring, float* physics_state, float* delayed) {
  if (!s) return SO101_ERR_ARG;
  if (!s->has_task) { s->err = "so101_tree_bind_physics_state: the model carries no task (bare-arm blob)"; return SO101_ERR_STATE; }
  bool all = ring && physics_state && delayed, none = !ring && !physics_state && !delayed;
  if (!all && !none) { s->err = "so101_tree_bind_physics_state: all three buffers or none"; return SO101_ERR_ARG; }
  s->env.ps_ring = ring; s->env.ps_out = physics_state; s->env.ps_delayed = delayed;
  return SO101_OK;
}

int TAPI(configure_env)(TreeHandle* s, const so101_tree_config* c) {
  if (!s || !c) return SO101_ERR_ARG;
  if (c->n_substeps < 1 || c->n_substeps > 1000 || c->last_step < 1 || c->settle_max_substeps < 0) { s->err = "so101_tree_configure_env: value out of range"; return SO101_ERR_ARG; }
  TreeTask& T = s->task;
  T.n_substeps = c->n_substeps; T.last_step = c->last_step; T.settle_max = c->settle_max_substeps; T.terminate_on_success = c->terminate_on_success;
  T.seed = c->seed; T.env_id_base = c->env_id_base;
  if (c->reward_mode < 0 || c->reward_mode > 2) { s->err = "so101_tree_configure_env: reward_mode must be 0, 1 or 2"; return SO101_ERR_ARG; }
  if (c->reward_mode != 0 && !s->hm.geom_class) { s->err = "so101_tree_configure_env: the model blob carries no task_geom_class (contact-sequence reward)"; return SO101_ERR_STATE; }
  T.reward_mode = c->reward_mode; T.requires_handover = c->reward_requires_handover;
  // observation delays in control steps; negative = the reference's defaults (0.1 s and 0.3 s at a 0.02 s control step)
  int jd = c->joints_delay_steps < 0 ? T_RING_DEFAULT : c->joints_delay_steps, pd = c->physics_delay_steps < 0 ? T_PS_DEFAULT : c->physics_delay_steps;
  if (jd > T_DELAY_MAX || pd > T_DELAY_MAX) { s->err = "so101_tree_configure_env: observation delay above 64 control steps"; return SO101_ERR_ARG; }
  T.jdelay = jd; T.pdelay = pd;
  // reset prefetch: whatever the cache holds was settled under the previous configuration
  {
    GUARD_DEVICE(s);
    if (!s->side.drain(s, "hipStreamSynchronize(prefetch)")) return SO101_ERR_HIP;
    s->prefetch = c->prefetch_resets != 0;
    if (s->prefetch && !tree_prefetch_setup(s)) return SO101_ERR_HIP;
    s->pipeline = c->pipeline != 0;
    if (s->pipeline && !tree_pipe_setup(s)) return SO101_ERR_HIP;
    if (s->ctag && !hip_ok(s, hipMemset(s->ctag, 0, (size_t)s->n_envs * sizeof(unsigned int)), "hipMemset(prefetch)")) return SO101_ERR_HIP;
  }
  return TAPI(configure)(s, c->solver_iterations, c->solver_tolerance);
}

int TAPI(reset)(TreeHandle* s, const uint8_t* mask, void* stream) {
  if (!s) return SO101_ERR_ARG;
  if (!s->bound || !s->env_bound) { s->err = "so101_tree_reset before so101_tree_bind_state / so101_tree_bind_env"; return SO101_ERR_STATE; }
  GUARD_DEVICE(s);
  hipLaunchKernelGGL(k_tree_reset, dim3(s->n_envs), dim3(64), 0, (hipStream_t)stream, s->dm, s->dg, task_now(s), s->buf, s->env, store_now(s), mask);
  if (!hip_ok(s, hipGetLastError(), "k_tree_reset")) return SO101_ERR_HIP;
  launch_tree_prepare(s, (hipStream_t)stream);
  return SO101_OK;
}

int TAPI(step)(TreeHandle* s, const float* action, float* obs, float* reward, float* discount, uint8_t* step_type, void* stream) {
  if (!s || !action || !obs || !reward || !discount || !step_type) { if (s) s->err = "so101_tree_step: NULL argument"; return SO101_ERR_ARG; }
  if (!s->bound || !s->env_bound) { s->err = "so101_tree_step before so101_tree_bind_state / so101_tree_bind_env"; return SO101_ERR_STATE; }
  GUARD_DEVICE(s);
  hipStream_t st = (hipStream_t)stream;
  TreeTask T = task_now(s);
  const bool post = T.reward_mode != 0;          // contact rewards: one more narrowphase launch, on the post-step state
  // what to launch is decided by the plan (so101_step_plan.hpp); this function executes it and counts what it enqueued
  const TreeStepPlan plan = plan_tree_step(s->n_envs, T.n_substeps, post, s->pipeline && s->pipe.pose, TreeHandle::MAXSLICES, TPIPE_MAXSUB, read_step_knobs());
  int launches = 0, memsets = 0;
  if (plan.chain) {
    // launch chain: prologue, then per substep the narrowphase of every candidate pair of the batch and the rest of the substep per env.
    // Env slices on their own streams: the narrowphase of one (latency-bound, two wavefronts per SIMD) runs beside the solve of another
    // (four envs per CU by its LDS footprint); the slices share nothing but the model.
    if (!s->slices.fork(s, st, plan.G)) return SO101_ERR_HIP;
    for (int g = 0; g < plan.G; g++) {
      const int e0 = plan.slice[g].e0, ng = plan.slice[g].ng, nw = plan.slice[g].nw;
      TreePipe P = s->pipe;
      P.counters = s->pipe.counters + 2 * TPIPE_MAXSUB * g;
      P.work = s->pipe.work + (size_t)2 * e0 * TCAND;
      P.work_cap = (unsigned int)ng * TCAND;
      hipStream_t gs;
      if (!s->slices.stream_of(s, g, &gs)) return SO101_ERR_HIP;
      if (!hip_ok(s, hipMemsetAsync(P.counters, 0, 2 * TPIPE_MAXSUB * sizeof(int), gs), "hipMemsetAsync(pipeline)")) return SO101_ERR_HIP;
      memsets++;
      hipLaunchKernelGGL(k_tree_pipe_begin, dim3(ng), dim3(64), 0, gs, s->dm, s->dg, T, s->buf, s->env, store_now(s), P, action, obs, reward, discount, step_type, e0);
      launches++;
      for (int k = 0; k < T.n_substeps; k++) {
        hipLaunchKernelGGL(k_tree_narrow, dim3(nw), dim3(64), 0, gs, s->dm, s->dg, P, s->n_envs, k);
        hipLaunchKernelGGL(k_tree_pipe_solve, dim3(ng), dim3(64), 0, gs, s->dm, s->dg, T, s->buf, s->env, P, k, (int)(!post && k == T.n_substeps - 1), obs, reward, discount, step_type, e0);
        launches += 2;
      }
      if (post) {
        hipLaunchKernelGGL(k_tree_narrow, dim3(nw), dim3(64), 0, gs, s->dm, s->dg, P, s->n_envs, T.n_substeps);
        hipLaunchKernelGGL(k_tree_pipe_finish, dim3(ng), dim3(64), 0, gs, s->dm, s->dg, T, s->buf, s->env, P, obs, reward, discount, step_type, e0);
        launches += 2;
      }
      if (!hip_ok(s, hipGetLastError(), "k_tree_pipe_solve")) return SO101_ERR_HIP;
      if (!s->slices.join(s, g)) return SO101_ERR_HIP;
    }
  } else {
    hipLaunchKernelGGL(k_tree_step, dim3(s->n_envs), dim3(64), 0, st, s->dm, s->dg, T, s->buf, s->env, store_now(s), action, obs, reward, discount, step_type);
    launches++;
    if (!hip_ok(s, hipGetLastError(), "k_tree_step")) return SO101_ERR_HIP;
  }
  // (a step that failed above leaves the plan of the last step that was enqueued whole)
  s->plan[0] = plan.G; s->plan[1] = launches; s->plan[2] = memsets; s->plan[3] = plan.chain ? 2 : 1;
  launch_tree_prepare(s, (hipStream_t)stream);
  return SO101_OK;
}

int TAPI(compute_settled)(TreeHandle* s, int first_episode, int count, float* qpos, float* qvel, float* warmstart, int32_t* flags, void* stream) {
  if (!s || !qpos || !qvel || !warmstart || !flags || first_episode < 0 || count <= 0) { if (s) s->err = "so101_tree_compute_settled: bad argument"; return SO101_ERR_ARG; }
  if (!s->has_task) { s->err = "so101_tree_compute_settled: the model carries no task"; return SO101_ERR_STATE; }
  GUARD_DEVICE(s);
  for (int k = 0; k < count; k++) {      // one launch per episode: the per-env scratch is used by one wavefront at a time
    hipLaunchKernelGGL(k_tree_settle_table, dim3(s->n_envs), dim3(64), 0, (hipStream_t)stream, s->dm, s->dg, task_now(s), s->buf, (unsigned int)(first_episode + k), k,
                       qpos, qvel, warmstart, flags);
    if (!hip_ok(s, hipGetLastError(), "k_tree_settle_table")) return SO101_ERR_HIP;
  }
  return SO101_OK;
}

int TAPI(set_settled_store)(TreeHandle* s, int first_episode, int count, const float* qpos, const float* qvel, const float* warmstart, const int32_t* flags) {
  if (!s) return SO101_ERR_ARG;
  if (count > 0 && (!qpos || !qvel || !warmstart || !flags || first_episode < 0)) { s->err = "so101_tree_set_settled_store: bad argument"; return SO101_ERR_ARG; }
  s->store = TreeStore{};
  if (count > 0) { s->store.qpos = qpos; s->store.qvel = qvel; s->store.warm = warmstart; s->store.flags = flags; s->store.first = first_episode; s->store.count = count; }
  return SO101_OK;
}

int TAPI(settle)(TreeHandle* s, void* stream) {
  if (!s) return SO101_ERR_ARG;
  if (!s->bound) { s->err = "so101_tree_settle before so101_tree_bind_state"; return SO101_ERR_STATE; }
  GUARD_DEVICE(s);
  hipLaunchKernelGGL(k_tree_settle, dim3(s->n_envs), dim3(64), 0, (hipStream_t)stream, s->dm, s->dg, task_now(s), s->buf);
  return hip_ok(s, hipGetLastError(), "k_tree_settle") ? SO101_OK : SO101_ERR_HIP;
}

int TAPI(begin_episode)(TreeHandle* s, void* stream) {
  if (!s) return SO101_ERR_ARG;
  if (!s->bound || !s->env_bound) { s->err = "so101_tree_begin_episode before so101_tree_bind_state / so101_tree_bind_env"; return SO101_ERR_STATE; }
  GUARD_DEVICE(s);
  hipLaunchKernelGGL(k_tree_begin, dim3(s->n_envs), dim3(64), 0, (hipStream_t)stream, s->dm, task_now(s), s->buf, s->env);
  return hip_ok(s, hipGetLastError(), "k_tree_begin") ? SO101_OK : SO101_ERR_HIP;
}

// ---- cameras and colour cameras (tree_render_call above)
int TAPI(set_hull_planes)(TreeHandle* s, const float* planes, const int32_t* plane_adr) {
  if (!s) return SO101_ERR_ARG;
  if (!planes || !plane_adr) { s->err = "so101_tree_set_hull_planes: NULL argument"; return SO101_ERR_ARG; }
  if (!check_hull_planes(s, "so101_tree_set_hull_planes", s->render, planes, plane_adr)) return SO101_ERR_ARG;          // (so101_host.hpp)
  GUARD_DEVICE(s);
  return s->render.upload_planes(s, planes, plane_adr) ? SO101_OK : SO101_ERR_HIP;
}

int TAPI(render)(TreeHandle* s, const so101_camera* cams, int ncam, int height, int width, const int32_t* env_index, int n_render, int source,
                 float* depth, int32_t* seg, void* stream) {
  return tree_render_call(s, "so101_tree_render", false, cams, ncam, height, width, env_index, n_render, source, nullptr, nullptr, 0, nullptr, depth, (int*)seg, stream);
}

int TAPI(render_color)(TreeHandle* s, const so101_camera* cams, int ncam, int height, int width, const int32_t* env_index, int n_render, int source,
                       const so101_shading* shading, const float* geom_rgb, int rgb_per_env, const so101_color_out* out, void* stream) {
  return tree_render_call(s, "so101_tree_render_color", true, cams, ncam, height, width, env_index, n_render, source, shading, geom_rgb, rgb_per_env, out, nullptr, nullptr, stream);
}

// ---- Cartesian tool control (so101_tool_chain.hpp)
int TAPI(tool_chain)(TreeHandle* s, int body, int32_t* dof, int32_t* qposadr, int32_t* jnt_type) {
  if (!s) return SO101_ERR_ARG;
  ToolChain<TREE_TOOL_MAXCOL> T;
  int d[TREE_TOOL_MAXCOL] = {};
  if (int rc = tree_tool_chain(s, "so101_tree_tool_chain", body, nullptr, T, d)) return rc;
  for (int k = 0; k < T.ncol; k++) {
    if (dof) dof[k] = d[k];
    if (qposadr) qposadr[k] = T.qposadr[k];
    if (jnt_type) jnt_type[k] = T.type[k];
  }
  return T.ncol;
}

int TAPI(ik_default_config)(TreeHandle* s, int body, so101_tree_ik_config* cfg) {
  if (!s || !cfg) return SO101_ERR_ARG;
  ToolChain<TREE_TOOL_MAXCOL> T;
  if (int rc = tree_tool_chain(s, "so101_tree_ik_default_config", body, nullptr, T, nullptr)) return rc;
  ik_default_settings(cfg);
  int k = T.ncol;
  for (int b = body; b != 0; b = s->hm.body_parent[b]) {          // the chain's joints, tool side first
    const int j = s->hm.body_jnt[b];
    if (j < 0) continue;
    k--;
    const bool limited = s->hm.jnt_limited[j] != 0;
    cfg->q_lo[k] = limited ? s->hm.jnt_range[j][0] : -3.0e38f; cfg->q_hi[k] = limited ? s->hm.jnt_range[j][1] : 3.0e38f;
    if (T.type[k] == TJ_HINGE) cfg->free_mask |= 1u << k;          // (slide joints - the fingers - are held by default)
  }
  return SO101_OK;
}

int TAPI(tool_pose)(TreeHandle* s, const so101_tree_tool* tool, const float* q, const int32_t* env_index, int n, float* pos, float* mat, float* jac, void* stream) {
  if (!s) return SO101_ERR_ARG;
  ToolChain<TREE_TOOL_MAXCOL> T;
  if (int rc = check_tool_frame(s, "so101_tree_tool_pose", tool)) return rc;
  if (int rc = tree_tool_chain(s, "so101_tree_tool_pose", tool->body, tool, T, nullptr)) return rc;
  if (int rc = check_tool_entries(s, "so101_tree_tool_pose", q != nullptr, env_index != nullptr, n, s->bound, s->n_envs)) return rc;
  if (!pos && !mat && !jac) { s->err = "so101_tree_tool_pose: no output (pos, mat and jac are all NULL)"; return SO101_ERR_ARG; }
  GUARD_DEVICE(s);
  so101::launch_tool_pose(n, (hipStream_t)stream, T, q, (const float*)s->buf.qpos, s->n_envs, (const int*)env_index, pos, mat, jac);
  return hip_ok(s, hipGetLastError(), "k_tool_pose") ? SO101_OK : SO101_ERR_HIP;
}

int TAPI(tool_ik)(TreeHandle* s, const so101_tree_tool* tool, const so101_tree_ik_config* cfg, const float* target_pos, const float* target_mat, const float* q_init,
                  const int32_t* env_index, int n, float* q_out, float* residual, int32_t* info, void* stream) {
  if (!s) return SO101_ERR_ARG;
  ToolChain<TREE_TOOL_MAXCOL> T;
  IkSettings<TREE_TOOL_MAXCOL> C;
  if (int rc = check_tool_frame(s, "so101_tree_tool_ik", tool)) return rc;
  if (int rc = tree_tool_chain(s, "so101_tree_tool_ik", tool->body, tool, T, nullptr)) return rc;
  if (int rc = check_tool_entries(s, "so101_tree_tool_ik", q_init != nullptr, env_index != nullptr, n, s->bound, s->n_envs)) return rc;
  if (int rc = ik_settings(s, "so101_tree_tool_ik", cfg, T.ncol, cfg ? cfg->free_mask : 0u, target_pos != nullptr, target_mat != nullptr, q_out != nullptr, C)) return rc;
  GUARD_DEVICE(s);
  so101::launch_tool_ik(n, (hipStream_t)stream, T, C, target_pos, target_mat, q_init, (const float*)s->buf.qpos, s->n_envs, (const int*)env_index, q_out, residual, (int*)info);
  return hip_ok(s, hipGetLastError(), "k_tool_ik") ? SO101_OK : SO101_ERR_HIP;
}

// ---- contact sensing (k_tree_contacts of so101_tree_kernels.hpp)
int TAPI(contacts)(TreeHandle* s, const int32_t* env_index, int n, int forces, const so101_tree_geom_pair* pairs, int npair, const so101_contact_out* out, void* stream) {
  if (!s) return SO101_ERR_ARG;
  const so101_contact_out* o = out;
  if (int rc = check_contact_arguments(s, "so101_tree_contacts", o, env_index != nullptr, n, s->n_envs, forces, pairs != nullptr, npair)) return rc;          // (so101_host.hpp)
  TouchPairsT<8> T{};
  if (int rc = pack_touch_pairs(s, "so101_tree_contacts", pairs, npair, s->hm.ngeom, T)) return rc;
  if (!s->bound) { s->err = "so101_tree_contacts: state buffers not bound (call so101_tree_bind_state)"; return SO101_ERR_STATE; }
  GUARD_DEVICE(s);
  const ContactOut O = contact_out_of(o);
  // with forces entry i works in scratch slice i mod n_envs (env_index may repeat an env): at most n_envs entries per launch, the launches in
  // stream order; without forces the scratch is not touched and one launch serves any n
  const int chunk = forces ? s->n_envs : n;
  for (int i0 = 0; i0 < n; i0 += chunk) {
    const int cnt = n - i0 < chunk ? n - i0 : chunk;
    hipLaunchKernelGGL(k_tree_contacts, dim3((unsigned int)cnt), dim3(64), 0, (hipStream_t)stream, s->dm, s->dg, s->buf, s->n_envs, s->iterations, s->tolerance, (const int*)env_index, i0,
                       (int)(forces != 0), T, O);
    if (!hip_ok(s, hipGetLastError(), "k_tree_contacts")) return SO101_ERR_HIP;
  }
  return SO101_OK;
}

// ---- proximity sensing (k_tree_proximity of so101_tree_kernels.hpp; the checks of so101_proximity in its order, then the columns of q)
int TAPI(proximity)(TreeHandle* s, const int32_t* env_index, int n, const float* q, const int32_t* q_adr, int ncol, const so101_tree_geom_pair* pairs, int npair, float max_dist,
                    const so101_proximity_out* out, void* stream) {
  if (!s) return SO101_ERR_ARG;
  const so101_proximity_out* o = out;
  if (int rc = check_proximity_arguments(s, "so101_tree_proximity", o, env_index != nullptr, n, s->n_envs, pairs != nullptr, npair)) return rc;          // (so101_host.hpp)
  TouchPairsT<8> T{};
  if (int rc = pack_touch_pairs(s, "so101_tree_proximity", pairs, npair, s->hm.ngeom, T)) return rc;
  if (!(std::isfinite(max_dist) && max_dist > 0.f && max_dist <= 10.f)) { s->err = "so101_tree_proximity: max_dist must be a finite number above 0 and at most 10"; return SO101_ERR_ARG; }
  ProxCols C{};
  const char* bad = nullptr;
  if (q && !q_adr) bad = "q without q_adr";
  else if (!q && q_adr) bad = "q_adr without q";
  else if (q && (ncol < 1 || ncol > PROX_MAXCOL)) bad = "ncol must be 1 .. 16";
  if (bad) { s->err = std::string("so101_tree_proximity: ") + bad; return SO101_ERR_ARG; }
  if (q) {
    C.ncol = ncol;
    for (int k = 0; k < ncol; k++) {
      bool joint = false;
      for (int b = 1; b < s->hm.nbody; b++)
        joint = joint || ((s->hm.body_jnttype[b] == TJ_HINGE || s->hm.body_jnttype[b] == TJ_SLIDE) && s->hm.body_qposadr[b] == q_adr[k]);
      if (!joint) {
        s->err = "so101_tree_proximity: q_adr[" + std::to_string(k) + "] = " + std::to_string(q_adr[k]) + " is not the qpos address of a hinge or slide joint";
        return SO101_ERR_ARG;
      }
      for (int j = 0; j < k; j++)
        if (q_adr[j] == q_adr[k]) {
          s->err = "so101_tree_proximity: q_adr[" + std::to_string(k) + "] repeats address " + std::to_string(q_adr[k]) + " of q_adr[" + std::to_string(j) + "]";
          return SO101_ERR_ARG;
        }
      C.adr[k] = q_adr[k];
    }
  }
  if (!s->bound) { s->err = "so101_tree_proximity: state buffers not bound (call so101_tree_bind_state)"; return SO101_ERR_STATE; }
  GUARD_DEVICE(s);
  hipLaunchKernelGGL(k_tree_proximity, dim3((unsigned int)n * (unsigned int)npair), dim3(64), 0, (hipStream_t)stream, s->dm, s->dg, s->buf, s->n_envs, (const int*)env_index, q, C, T,
                     max_dist, ProxOut{o->dist, (int*)o->geom, o->point, o->normal, (int*)o->flags, (int*)o->queries});
  return hip_ok(s, hipGetLastError(), "k_tree_proximity") ? SO101_OK : SO101_ERR_HIP;
}

int TAPI(get_diag)(TreeHandle* s, int* out /* [n_envs][8] device or host-visible memory */, void* stream) {
  if (!s || !out) return SO101_ERR_ARG;
  GUARD_DEVICE(s);
  return hip_ok(s, hipMemcpyAsync(out, s->buf.diag, (size_t)s->n_envs * 8 * sizeof(int), hipMemcpyDefault, (hipStream_t)stream), "hipMemcpyAsync(diag)") ? SO101_OK : SO101_ERR_HIP;
}

}  // extern "C"
}  // namespace TREE_NS
