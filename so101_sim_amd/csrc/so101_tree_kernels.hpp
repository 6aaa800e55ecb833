// General-tree engine: the kernels over the device functions of so101_tree.hpp, launched by tu_tree.hip and so101_tree_host.hpp.  Included
// once per build of the engine (TREE_VARIANT): no include guard, every macro is undefined before it is defined.
// so101_tree_debug_forward layout (floats per env; dims[7..14] of so101_tree_dims report it): counts, bias, qacc_smooth, qacc [TV each],
// body positions [TB][3], mass matrix [TV][TV], contacts [TCON][10] (pos3 normal3 dist geom1 geom2 dim), normal forces [TCON]
#include "so101_contact_report.hpp"      // (guarded: the report tail of k_tree_contacts is one template for both builds)
#include "so101_proximity_core.hpp"      // (guarded: the distance code of k_tree_proximity is the SO100 engine's)
#undef TDBG_COUNTS
#undef TDBG_BIAS
#undef TDBG_QSM
#undef TDBG_QACC
#undef TDBG_XPOS
#undef TDBG_M
#undef TDBG_CON
#undef TDBG_FORCE
#undef TDBG_DIM
#define TDBG_COUNTS 0        // ncon, nrow, iters, ncand, flags, nscalar
#define TDBG_BIAS 8
#define TDBG_QSM (TDBG_BIAS + TV)
#define TDBG_QACC (TDBG_QSM + TV)
#define TDBG_XPOS (TDBG_QACC + TV)     // [TB][3]
#define TDBG_M (TDBG_XPOS + 3 * TB)    // [TV][TV]
#define TDBG_CON (TDBG_M + TV * TV)    // [TCON][10]
#define TDBG_FORCE (TDBG_CON + 10 * TCON)
#define TDBG_DIM (((TDBG_FORCE + TCON) + 63) / 64 * 64)

namespace TREE_NS {
using tree::TreePipe;

__global__ void __launch_bounds__(64) k_tree_physics(const TreeModel* tm, const DevModel* gm, TreeBuffers B, int N, int nsub, int iterations, float tolerance) {
  BLOCK_SHARED(TreeLDS, L);
  int e = blockIdx.x, lane = wave_lane();
  if (lane == 0) L.flags = 0;
  tree::load_state(tm, L, B, e, N);
  TreeScratch G = tree::scratch_of(B, e);
  int bad = 0;
  for (int s = 0; s < nsub; s++) {
    tree::forward(tm, gm, L, G, iterations, tolerance);
    tree::euler(tm, L);
    if (tree::diverged(tm, L)) { bad = 1; break; }
  }
  if (lane == 0 && bad) L.flags |= 8;
  tree::store_state(tm, L, B, e, N);
  if (lane == 0) tree::store_diag(B, L, e);
}

__global__ void __launch_bounds__(64) k_tree_forward(const TreeModel* tm, const DevModel* gm, TreeBuffers B, int N, int iterations, float tolerance, float* out, int phases) {
  BLOCK_SHARED(TreeLDS, L);
  int e = blockIdx.x, lane = wave_lane();
  if (lane == 0) L.flags = 0;
#ifdef TREE_PROF
  if (lane < 32) L.prof[lane] = 0u;
#endif
  tree::load_state(tm, L, B, e, N);
  TreeScratch G = tree::scratch_of(B, e);
  tree::forward(tm, gm, L, G, iterations, tolerance, phases);
  float* o = out + (size_t)e * TDBG_DIM;
  int nv = tm->nv, nb = tm->nbody;
  if (lane == 0) { o[0] = (float)L.ncon; o[1] = (float)L.nrow; o[2] = (float)L.iters; o[3] = (float)L.ncand; o[4] = (float)L.flags; o[5] = (float)L.nscalar; }
  if (lane < nv) {
    o[TDBG_BIAS + lane] = L.bias[lane]; o[TDBG_QSM + lane] = L.qsm[lane]; o[TDBG_QACC + lane] = L.qacc[lane];
    for (int r = 0; r < nv; r++) o[TDBG_M + r * TV + lane] = L.M[r][lane];
  }
  if (lane < nb) for (int k = 0; k < 3; k++) o[TDBG_XPOS + 3 * lane + k] = L.xpos[lane][k];
#ifdef TREE_PROF
  wave_sync();
  if (lane < 16) o[TDBG_M + lane] = (float)L.prof[lane];         // (profiling variant: the phase clocks take the first slots of the mass-matrix dump)
#endif
  for (int ci = lane; ci < L.ncon; ci += WAVE) {
    const TCon& c = L.con[ci];
    float* q = o + TDBG_CON + 10 * ci;
    for (int k = 0; k < 3; k++) { q[k] = c.pos[k]; q[3 + k] = c.frame[k]; }
    q[6] = c.dist; q[7] = (float)c.g1; q[8] = (float)c.g2; q[9] = (float)c.dim;
    o[TDBG_FORCE + ci] = L.nrow > 0 ? G.ef[c.row] : 0.f;
  }
}

// env.reset() of the envs whose mask byte is set (NULL: all), then the FIRST observation is what the next step call reports
__global__ void __launch_bounds__(64) k_tree_reset(const TreeModel* tm, const DevModel* gm, TreeTask T, TreeBuffers B, TreeEnvBuffers E, TreeStore S, const unsigned char* mask) {
  BLOCK_SHARED(TreeLDS, L);
  int e = blockIdx.x, lane = wave_lane(), N = T.n_envs;
  if (mask && !mask[e]) return;
  if (lane == 0) L.flags = 0;
  wave_sync();
  TreeScratch G = tree::scratch_of(B, e);
  tree::env_reset(tm, gm, T, L, G, B, E, S, e);
  tree::store_state(tm, L, B, e, N);
  if (lane < tm->nu) B.ctrl[(size_t)lane * N + e] = L.ctrl[lane];
  if (lane == 0) { E.need_reset[e] = 0; tree::store_diag(B, L, e); }
}

// placement + settle of episode `episode` of every env into row k of caller-owned tables (so101_tree_compute_settled): what env_reset()
// would compute for that episode, without touching any env state
__global__ void __launch_bounds__(64) k_tree_settle_table(const TreeModel* tm, const DevModel* gm, TreeTask T, TreeBuffers B, unsigned int episode, int k,
                                                          float* qpos, float* qvel, float* warm, int* flags) {
  BLOCK_SHARED(TreeLDS, L);
  int e = blockIdx.x, lane = wave_lane(), N = T.n_envs;
  if (lane == 0) L.flags = 0;
  wave_sync();
  TreeScratch G = tree::scratch_of(B, e);
  tree::env_settle(tm, gm, T, L, G, e, episode);
  size_t kk = (size_t)k;
  if (lane < tm->nq) qpos[(kk * tm->nq + lane) * N + e] = L.qpos[lane];
  if (lane < tm->nv) { qvel[(kk * tm->nv + lane) * N + e] = L.qvel[lane]; warm[(kk * tm->nv + lane) * N + e] = L.warm[lane]; }
  if (lane == 0) flags[kk * N + e] = L.flags;
}

// Reset prefetch: the settled state of the NEXT episode of every env whose cache entry does not hold it yet (TreeStore, so101_tree.hpp), into
// the library's cache, on a low-priority stream beside the stepping kernels; its own per-env scratch (B.scratch here is the second one)
__global__ void __launch_bounds__(64) k_tree_prepare(const TreeModel* tm, const DevModel* gm, TreeTask T, TreeBuffers B, const int* episode_of, TreeStore S) {
  BLOCK_SHARED(TreeLDS, L);
  int e = blockIdx.x, lane = wave_lane(), N = T.n_envs;
  unsigned int episode = (unsigned int)ld_agent(&episode_of[e]);
  if (ld_agent(&S.ctag[e]) == episode + 1u) return;                                      // the entry is current
  if (S.qpos && episode - (unsigned int)S.first < (unsigned int)S.count) return;          // the caller's settled-state store covers it
  if (lane == 0) L.flags = 0;
  wave_sync();
  TreeScratch G = tree::scratch_of(B, e);
  tree::env_settle(tm, gm, T, L, G, e, episode);
  if (lane == 0) st_agent(&S.ctag[e], 0u);                                                 // (no reader may take a half-written entry for the old episode)
  drain_stores();
  if (lane < tm->nq) st_agent(&S.cq[(size_t)lane * N + e], L.qpos[lane]);
  if (lane < tm->nv) { st_agent(&S.cv[(size_t)lane * N + e], L.qvel[lane]); st_agent(&S.cw[(size_t)lane * N + e], L.warm[lane]); }
  if (lane == 0) st_agent(&S.cf[e], L.flags);
  drain_stores();
  wave_sync();
  if (lane == 0) st_agent(&S.ctag[e], episode + 1u);
}

// settle the bound state with the one-dof joints held (dm_control's PropPlacer(settle_physics=True) alone, for callers that draw the
// placements themselves): until |qvel| < 1e-3 and |qacc| < 1e-2 over the props' dofs or the budget ends (flag 32)
__global__ void __launch_bounds__(64) k_tree_settle(const TreeModel* tm, const DevModel* gm, TreeTask T, TreeBuffers B) {
  BLOCK_SHARED(TreeLDS, L);
  int e = blockIdx.x, lane = wave_lane(), N = T.n_envs;
  if (lane == 0) L.flags = 0;
  tree::load_state(tm, L, B, e, N);
  TreeScratch G = tree::scratch_of(B, e);
  float q0 = lane < tm->njnt ? L.qpos[lane] : 0.f, v0 = lane < tm->njnt ? L.qvel[lane] : 0.f;
  bool settled = T.settle_max == 0;
  for (int k = 0; k < T.settle_max && !settled; k++) {
    tree::forward(tm, gm, L, G, T.iterations, T.tolerance);
    tree::euler(tm, L);
    bool bad = tree::diverged(tm, L);       // (a named bool, as in tree::env_settle)
    if (bad) { if (lane == 0) L.flags |= 8; break; }
    if (lane < tm->njnt) { L.qpos[lane] = q0; L.qvel[lane] = v0; }
    wave_sync();
    float mv = 0.f, ma = 0.f;
    if (lane >= tm->njnt && lane < tm->nv) { mv = fabsf(L.qvel[lane]); ma = fabsf(L.qacc[lane]); }
    mv = wave_max_f(mv); ma = wave_max_f(ma);
    settled = mv < 1e-3f && ma < 1e-2f;
  }
  if (!settled && lane == 0) L.flags |= 32;
  tree::store_state(tm, L, B, e, N);
  if (lane == 0 && B.diag) tree::store_diag(B, L, e);       // (B.diag tested here too: without it this kernel's register allocation changes)
}

// adopt the bound state as the post-reset state of a new episode (known-answer tests, checkpoints): delay lines filled with it,
// counters cleared, no reset pending
__global__ void __launch_bounds__(64) k_tree_begin(const TreeModel* tm, TreeTask T, TreeBuffers B, TreeEnvBuffers E) {
  BLOCK_SHARED(TreeLDS, L);
  int e = blockIdx.x, lane = wave_lane(), N = T.n_envs;
  tree::load_state(tm, L, B, e, N);
  tree::fill_delay_lines(tm, T, L, E, e);
  if (lane == 0) { E.step_count[e] = 0; E.ep_return[e] = 0.f; E.need_reset[e] = 0; E.success_state[e] = T.requires_handover ? 0 : 2; }
}

// end of a control step of one env (after the last substep): observation, reward / discount / termination, state and counters out
// CONTACTS: where the contact rewards take the contacts of the post-step state from - 0: not compiled (reward mode 0 only), 1: collision() in
// place (single kernel), 2: gathered from the launch chain's records (k_tree_pipe_finish)
template <int CONTACTS>
__device__ __forceinline__ void tree_finish_step(const TreeModel* tm, const DevModel* gm, const TreeTask& T, TreeLDS& L, TreeScratch& G, const TreeBuffers& B,
                                                 const TreeEnvBuffers& E, int e, bool diverged, float* obs, float* reward, float* discount, unsigned char* step_type,
                                                 const TreePipe* P = nullptr) {
  int lane = wave_lane(), N = T.n_envs;
  if (diverged) {         // mj_check*: the data is reset, dm_control ends the episode with reward 0 and discount 0
    if (lane < tm->nq) L.qpos[lane] = 0.f;
    if (lane < tm->nv) { L.qvel[lane] = 0.f; L.warm[lane] = 0.f; }
    wave_sync();
    if (lane > 0 && lane < tm->nbody && tm->body_jnttype[lane] == TJ_FREE) L.qpos[tm->body_qposadr[lane] + 3] = 1.f;
    if (lane == 0) L.flags |= 8;
    wave_sync();
  }
  int sc = E.step_count[e] + 1;
  tree::kinematics(tm, L);
  tree::write_obs(T, L, E, e, sc, false, obs);
  tree::write_physics_state(tm, T, L, E, e, sc);
  // dm_control's Environment.step asks the task three times: get_reward, get_discount (-> should_terminate_episode -> get_reward) and
  // should_terminate_episode (-> get_reward), aloha2_task.py:353-367.  For the overlap and touching rewards the three answers are the
  // same; the contact sequence (hand_over.py:286-338) advances its state machine on EVERY call, so reward, discount and termination may
  // each see a different state (0 -> 1 -> 2 and even the success within one control step).  Contacts: physics.data.contact after
  // physics.step(), whose legacy step ends with mj_step1 - the contacts of the integrated state, recomputed here.
  float r = 0.f, r_disc = 0.f, r_term = 0.f;
  if (!diverged) {
    if (CONTACTS == 0 || T.reward_mode == 0) r = r_disc = r_term = tree::task_reward(tm, T, L);
    else if (T.reward_mode == 2) {
      if constexpr (CONTACTS == 2) tree::gather_contacts(tm, gm, L, *P, e); else tree::collision(tm, gm, L);
      r = r_disc = r_term = tree::task_reward_touching(tm, T, L);
    } else {
      if constexpr (CONTACTS == 2) tree::gather_contacts(tm, gm, L, *P, e); else tree::collision(tm, gm, L);
      int st = E.success_state[e];
      r = tree::task_reward_contacts(tm, T, L, G, &st);
      if (T.terminate_on_success) { r_disc = tree::task_reward_contacts(tm, T, L, G, &st); r_term = tree::task_reward_contacts(tm, T, L, G, &st); }
      if (lane == 0) E.success_state[e] = st;
    }
  }
  bool disc0 = (T.terminate_on_success && r_disc >= 1.f) || diverged, success = (T.terminate_on_success && r_term >= 1.f) || diverged, timeout = sc >= T.last_step;
  tree::store_state(tm, L, B, e, N);
  if (lane < tm->nu) B.ctrl[(size_t)lane * N + e] = L.ctrl[lane];
  if (lane == 0) {
    reward[e] = r; discount[e] = disc0 ? 0.f : 1.f;
    unsigned char st = (success || timeout) ? 2 : 1;
    step_type[e] = st; E.need_reset[e] = st == 2;
    E.step_count[e] = sc; E.ep_return[e] += r;
    tree::store_diag(B, L, e);
    if (B.diag) B.diag[8 * e + 5] = E.success_state[e];
  }
}

// start of a control step of one env: an env whose last step was LAST resets and reports FIRST (returns true: done for this call);
// the others load their state and apply the action
__device__ __forceinline__ bool tree_begin_step(const TreeModel* tm, const DevModel* gm, const TreeTask& T, TreeLDS& L, TreeScratch& G, const TreeBuffers& B,
                                                const TreeEnvBuffers& E, const TreeStore& S, int e, const float* action, float* obs, float* reward, float* discount,
                                                unsigned char* step_type) {
  int lane = wave_lane(), N = T.n_envs;
  if (E.need_reset[e]) {
    tree::env_reset(tm, gm, T, L, G, B, E, S, e);
    tree::kinematics(tm, L);
    tree::write_obs(T, L, E, e, 0, true, obs);
    tree::store_state(tm, L, B, e, N);
    if (lane < tm->nu) B.ctrl[(size_t)lane * N + e] = L.ctrl[lane];
    if (lane == 0) { reward[e] = 0.f; discount[e] = 1.f; step_type[e] = 0; E.need_reset[e] = 0; }
    if (lane == 0) tree::store_diag(B, L, e);
    return true;
  }
  tree::load_state(tm, L, B, e, N);
  // before_step (aloha2_task.py:316-349): joint targets as given, grippers from follower units to the sim's ctrl range; no clipping
  if (lane < tm->nu) {
    float a = action[(size_t)e * tm->nu + lane];
    if (T.act_is_gripper[lane]) a = tree::convert_gripper(a, T.grip[4], T.grip[5], T.grip[2], T.grip[3]);
    L.ctrl[lane] = a;
  }
  wave_sync();
  return false;
}

// (The single-kernel step: N = 1, steps of more than 63 substeps, and the reference the launch chain below is tested against.  One wavefront per
// SIMD: 458 unified registers, the hull caches and the EPA polytope of the inlined narrowphase among them.  __launch_bounds__(64, 2) was measured
// in round 4 - 256 VGPRs, 770 spilled, 864 B of scratch per lane: 171 k against 175 k env-steps/s at 4096 envs.)
// one control step of every env: dm_control's Environment.step - an env whose last step was LAST resets and reports FIRST
// (the action is ignored), the others apply the action, run n_substeps and report observation, reward, discount, step type
__global__ void __launch_bounds__(64) k_tree_step(const TreeModel* tm, const DevModel* gm, TreeTask T, TreeBuffers B, TreeEnvBuffers E, TreeStore S, const float* action,
                                                  float* obs, float* reward, float* discount, unsigned char* step_type) {
  BLOCK_SHARED(TreeLDS, L);
  int e = blockIdx.x, lane = wave_lane(), N = T.n_envs;
  if (lane == 0) L.flags = 0;
  wave_sync();
  TreeScratch G = tree::scratch_of(B, e);
  if (tree_begin_step(tm, gm, T, L, G, B, E, S, e, action, obs, reward, discount, step_type)) return;
  bool diverged = false;
  for (int s = 0; s < T.n_substeps && !diverged; s++) {
    tree::forward(tm, gm, L, G, T.iterations, T.tolerance);
    tree::euler(tm, L);
    diverged = tree::diverged(tm, L);
  }
  tree_finish_step<1>(tm, gm, T, L, G, B, E, e, diverged, obs, reward, discount, step_type);
}

#ifdef TREE_PROF
__device__ unsigned long long g_tprof[33];     // (profiling variant: phase clocks of k_tree_pipe_solve summed over env-substeps, printed by destroy)
#endif
// ---- the control step as a launch chain (so101_tree.hpp, "the narrowphase in a launch of its own"): k_tree_pipe_begin, then per substep
// k_tree_narrow and k_tree_pipe_solve.  Reward mode 0 (overlap boxes) only: the contact rewards need the contacts of the post-step state.
__global__ void __launch_bounds__(64) k_tree_pipe_begin(const TreeModel* tm, const DevModel* gm, TreeTask T, TreeBuffers B, TreeEnvBuffers E, TreeStore S, TreePipe P,
                                                        const float* action, float* obs, float* reward, float* discount, unsigned char* step_type, int e0) {
  BLOCK_SHARED(TreeLDS, L);
  int e = e0 + blockIdx.x, lane = wave_lane(), N = T.n_envs;
  if (lane == 0) L.flags = 0;
  wave_sync();
  TreeScratch G = tree::scratch_of(B, e);
  if (tree_begin_step(tm, gm, T, L, G, B, E, S, e, action, obs, reward, discount, step_type)) {
    if (lane == 0) { P.active[e] = 0; P.ncand[e] = 0; }
    return;
  }
  if (lane < tm->nu) B.ctrl[(size_t)lane * N + e] = L.ctrl[lane];
  if (lane == 0) { P.active[e] = 1; P.pflags[e] = 0; }
  tree::kinematics(tm, L);
  tree::publish(tm, gm, L, P, e, N, 0);
}

// one wavefront per candidate pair of the whole batch: persistent wavefronts take two work items per fetch
// (round 5: the hulls of a pair are staged in LDS - so101_geom.hpp, HullLDS - instead of held in 48 VGPRs; with the hull patches inlined the register
//  cache left this kernel 55 spilled VGPRs and 184 B of scratch per lane)
__global__ void __launch_bounds__(64, 2) k_tree_narrow(const TreeModel* tm, const DevModel* gm, TreePipe P, int N, int s) {
  __shared__ __attribute__((aligned(16))) float pool[3 * 2 * HULL_LDS_MAX];
  int lane = wave_lane();
  const int nwork = ldc(&P.counters[2 * s]);
  const unsigned int* list = P.work + (size_t)(s & 1) * P.work_cap;
  for (;;) {
    int i0 = 0;
    if (lane == 0) i0 = atomicAdd(&P.counters[2 * s + 1], 2);
    i0 = wave_uniform_i(i0);
    if (i0 >= nwork) break;
    unsigned int wl = 0, cl = 0;
    if (lane < 2 && i0 + lane < nwork) { wl = list[i0 + lane]; cl = P.cand[wl]; }
#pragma unroll 1
    for (int j = 0; j < 2; j++) {
      if (i0 + j >= nwork) break;
      unsigned int w = (unsigned int)__builtin_amdgcn_readlane((int)wl, j), c = (unsigned int)__builtin_amdgcn_readlane((int)cl, j);
      int e = (int)(w / TCAND), g1 = (int)(c & 0xffffu), g2 = (int)(c >> 16);
      int b1 = wave_uniform_i(tm->geom_body[g1]), b2 = wave_uniform_i(tm->geom_body[g2]);
      const float* p1 = P.pose + ((size_t)e * TB + b1) * 12; const float* p2 = P.pose + ((size_t)e * TB + b2) * 12;
      GeomW G1, G2;
      load_geom_at(gm, g1, p1, p1 + 3, G1); load_geom_at(gm, g2, p2, p2 + 3, G2);
      PairContacts pc;
      HullLDS H1{pool, hull_lds_slots(G1.type, G1.vnum)}, H2{pool + 3 * HULL_LDS_MAX, hull_lds_slots(G2.type, G2.vnum)};
      wave_sync();                                     // (the scans of the previous pair are done)
      hull_load(gm, G1, H1); hull_load(gm, G2, H2);
      wave_sync();
      narrow_pair_cached<HullLDS, G64>(gm, G1, G2, ldc(ldc(&gm->geom_rbound) + g1), ldc(ldc(&gm->geom_rbound) + g2), H1, H2, pc);
      if (lane == 0) {
        float* r = P.rec + (size_t)w * TREC;
        r[0] = (float)__popc(pc.valid); r[1] = pc.nrm[0]; r[2] = pc.nrm[1]; r[3] = pc.nrm[2];
        int o = 4;                                     // valid slots are written compactly, in slot order
#pragma unroll
        for (int q = 0; q < NCPP; q++)
          if ((pc.valid >> q) & 1u) { r[o] = pc.dist[q]; r[o + 1] = pc.pos[q][0]; r[o + 2] = pc.pos[q][1]; r[o + 3] = pc.pos[q][2]; o += 4; }
      }
    }
  }
}

__global__ void __launch_bounds__(64, TREE_SOLVE_OCC) k_tree_pipe_solve(const TreeModel* tm, const DevModel* gm, TreeTask T, TreeBuffers B, TreeEnvBuffers E, TreePipe P, int s, int last,
                                                                       float* obs, float* reward, float* discount, unsigned char* step_type, int e0) {
  BLOCK_SHARED(TreeLDS, L);
  int e = e0 + blockIdx.x, lane = wave_lane(), N = T.n_envs;
  int act = P.active[e];
  if (act == 0) return;
  if (lane == 0) L.flags = P.pflags[e];
#ifdef TREE_PROF
  if (lane < 32) L.prof[lane] = 0u;
  wave_sync();
#endif
  TPROF_T0();
  tree::load_state(tm, L, B, e, N);
  TPROF(16)
  TreeScratch G = tree::scratch_of(B, e);
  bool diverged = act == 2;
  if (!diverged) {
    tree::forward_smooth(tm, L);
    TPROF(12)
    tree::gather_contacts(tm, gm, L, P, e);
    TPROF(21)
    tree::forward_constrained(tm, L, G, T.iterations, T.tolerance);
    TPROF(13)
    tree::euler(tm, L);
    diverged = tree::diverged(tm, L);
    if (diverged && lane == 0) P.active[e] = 2;
    TPROF(22)
  }
  if (!last) {
    if (act == 1) {
      tree::store_state(tm, L, B, e, N);
      if (lane == 0) tree::save_pipe_diag(P, L, e);
      TPROF(23)
      if (!diverged) {
        tree::kinematics(tm, L);
        TPROF(24)
        tree::publish(tm, gm, L, P, e, N, s + 1);
        TPROF(25)
      }
      else if (lane == 0) P.ncand[e] = 0;
    }
#ifdef TREE_PROF
    wave_sync();
    if (lane < 32) atomicAdd(&g_tprof[lane], (unsigned long long)L.prof[lane]);
    if (lane == 0) atomicAdd(&g_tprof[32], 1ull);
#endif
    return;
  }
  if (act == 2) {
    // diverged in an earlier substep: this launch computed nothing, the diagnostics are those of the last substep that was
    if (lane == 0) tree::load_pipe_diag(P, L, e);
    wave_sync();
  }
  tree_finish_step<0>(tm, gm, T, L, G, B, E, e, diverged, obs, reward, discount, step_type);
}

// end of a control step whose reward needs the contacts of the post-step state (reward modes 1 and 2): the last k_tree_pipe_solve published that
// state's candidates like a substep's, k_tree_narrow has turned them into records
__global__ void __launch_bounds__(64, 2) k_tree_pipe_finish(const TreeModel* tm, const DevModel* gm, TreeTask T, TreeBuffers B, TreeEnvBuffers E, TreePipe P,
                                                            float* obs, float* reward, float* discount, unsigned char* step_type, int e0) {
  BLOCK_SHARED(TreeLDS, L);
  int e = e0 + blockIdx.x, lane = wave_lane(), N = T.n_envs;
  int act = P.active[e];
  if (act == 0) return;
  if (lane == 0) { L.flags = P.pflags[e]; tree::load_pipe_diag(P, L, e); }
  tree::load_state(tm, L, B, e, N);
  TreeScratch G = tree::scratch_of(B, e);
  tree_finish_step<2>(tm, gm, T, L, G, B, E, e, act == 2, obs, reward, discount, step_type, &P);
}

// ---- depth / segmentation cameras (so101_tree_render of include/so101.h): the frames kernel of this engine, one wavefront per rendered env.
// It runs the engine's own kinematics on the qpos of the selected source - q[lane * lane_stride + e * env_stride]: the bound state
// (qpos[nq][N], env-fastest) or the delayed physics-state line ([N][nq + nv], its first nq entries) - and publishes what k_render
// (so101_raycast.hpp) consumes, record for record as k_render_frames (so101_camera.hpp) does for SO100: per geom the world frame of
// load_geom_at(), the bounding-sphere centre and geom_rbound (-1: the env index is outside [0, N), nothing of that image can be hit), per
// camera its world frame.  A camera is fixed to the world (body -1 or 0: kinematics() keeps the identity there) or to a tree body.
__global__ void __launch_bounds__(64) k_tree_render_frames(const TreeModel* tm, const DevModel* gm, const float* q, size_t lane_stride, size_t env_stride, int N,
                                                           const int* env_index, RenderCams cams, int ncam, float* frames, float* camframes) {
  BLOCK_SHARED(TreeLDS, L);
  const int i = blockIdx.x, lane = wave_lane();
  int e = env_index ? env_index[i] : i;
  e = wave_uniform_i(e);
  const bool ok = e >= 0 && e < N;
  if (lane < tm->nq) L.qpos[lane] = q[(size_t)lane * lane_stride + (size_t)(ok ? e : 0) * env_stride];
  wave_sync();
  tree::kinematics(tm, L);
  const int ngeom = gm->ngeom;
  for (int g = lane; g < ngeom; g += WAVE) {
    int b = gm->geom_dyn[g];            // (this engine's geom_dyn is the body id)
    GeomW G;
    load_geom_at<G16>(gm, g, L.xpos[b], L.xmat[b], G);
    float* f = frames + ((size_t)i * ngeom + g) * RENDER_FRAME;
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = G.R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) { f[9 + k] = G.p[k]; f[12 + k] = G.c[k]; }
    f[15] = ok ? gm->geom_rbound[g] : -1.f;
  }
  // cameras: composed with their body's pose on wave-uniform values (constant indices into the kernel argument), lane 0 publishes
#pragma unroll
  for (int k = 0; k < RENDER_MAXCAM; k++) {
    if (k >= ncam) break;
    const int b = cams.cam[k].body < 0 ? 0 : cams.cam[k].body;
    float X[9], P0[3], cp[3], cm[9];
#pragma unroll
    for (int j = 0; j < 9; j++) { X[j] = L.xmat[b][j]; cm[j] = cams.cam[k].mat[j]; }
#pragma unroll
    for (int j = 0; j < 3; j++) { P0[j] = L.xpos[b][j]; cp[j] = cams.cam[k].pos[j]; }
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

// ---- contact sensing (so101_tree_contacts of include/so101.h): the contact list of an env's CURRENT bound state and its reduction over pairs of
// geom groups, one wavefront per reported entry.  The pass is tree::forward() cut down to the report, its stages in forward()'s order - which is
// what makes the numbers bit-identical to k_tree_forward's dump: load_state, kinematics; with `forces` crba, rne_bias, smooth; collision; with
// `forces` make_constraints and solve_newton with the handle's iterations and tolerance.  `forces` is a kernel argument: the branch is
// wave-uniform, and without it none of the dynamics runs.  Nothing is stored back - no store_state, no store_diag, the warmstart is read and left
// alone.  Everything after the pass is contact_report() of so101_contact_report.hpp, shared with the SO100 engine.
//
// Where the numbers come from (TreeContactView):
//   * TCon::frame is the FULL frame: write_contact() puts the normal (geom1 -> geom2) into row 0 and make_frame() completes rows 1 and 2.
//   * count and the per-contact geometry are those after collision(), read before make_constraints() runs: make_constraints() lowers L.ncon when
//     the rows of the last contacts do not fit TROW (flag 4).  Geometry with and without forces is therefore the same, bit for bit; the
//     contacts that got no rows (k >= nkeep) report zero force and add nothing to the sums.
//   * force[j] = G.ef[c.row + j] for j < c.dim, zero beyond - read through the TreeScratch the solve used (use_row_storage() may have moved the
//     rows into LDS) - and only when the pass has rows at all (nrow > 0, as k_tree_forward's TDBG_FORCE): without rows solve_newton() returns
//     before anything writes ef.
//   * L.flags, started at 0, is the flag word of THIS pass: 1 candidate overflow, 2 contact overflow (collision() ends the list at the first
//     pair that does not fit), with forces 4 (contacts dropped for rows).
//
// Scratch: make_constraints() and solve_newton() work in a per-env slice of B.scratch.  env_index may name an env more than once, and two
// wavefronts on one slice would race: entry i works in slice i mod n_envs, and the host enqueues at most n_envs entries per launch
// (tu_tree.hip).  No kernel of this engine reads scratch it did not write in the same launch, so whose slice it is does not matter.
struct TreeContactView {
  static constexpr int DIST = (int)(offsetof(TCon, dist) / 4), POS = (int)(offsetof(TCon, pos) / 4), FRAME = (int)(offsetof(TCon, frame) / 4);
  const TreeLDS& L;
  const TreeScratch& G;
  int count, flags, nkeep;
  bool solved;
  DEV int g1(int k) const { return L.con[k].g1; }
  DEV int g2(int k) const { return L.con[k].g2; }
  DEV const float* words(int k) const { return (const float*)&L.con[k]; }
  DEV float force(int k, int j) const { return solved && k < nkeep && j < L.con[k].dim ? G.ef[L.con[k].row + j] : 0.f; }
};

// entries i0 .. i0 + gridDim.x - 1 of the call; with forces at most N of them per launch (the scratch slices)
__global__ void __launch_bounds__(64) k_tree_contacts(const TreeModel* tm, const DevModel* gm, TreeBuffers B, int N, int iterations, float tolerance, const int* env_index, int i0,
                                                      int forces, TouchPairsT<8> T, ContactOut O) {
  BLOCK_SHARED(TreeLDS, L);
  const size_t i = (size_t)i0 + blockIdx.x;
  const int e = env_index ? wave_uniform_i(env_index[i]) : (int)i;
  if (e < 0 || e >= N) { contacts_outside<TCON>(i, T.npair, O); return; }
  if (wave_lane() == 0) L.flags = 0;
  tree::load_state(tm, L, B, e, N);
  tree::kinematics(tm, L);
  if (forces) {                     // (wave-uniform: a kernel argument)
    tree::crba(tm, L);
    tree::rne_bias(tm, L);
    tree::smooth(tm, L);
  }
  tree::collision(tm, gm, L);
  const int ncon = L.ncon;          // the list of collision(): make_constraints() may shorten it
  int nkeep = ncon, nrow = 0;
  TreeScratch G = tree::scratch_of(B, (int)(i % (size_t)N));
  if (forces) {
    tree::make_constraints(tm, L, G);
    tree::solve_newton(tm, L, G, iterations, tolerance);
    nkeep = L.ncon; nrow = L.nrow;
  }
  wave_sync();
  contact_report<TCON>(i, TreeContactView{L, G, ncon, L.flags, nkeep, forces && nrow > 0}, forces != 0, T, O);
}

// ---- proximity sensing (so101_tree_proximity of include/so101.h): k_proximity of the SO100 engine (so101_proximity.hpp) on this engine's state, one
// wavefront per (entry, group pair); candidates, bounds, the exact query and the output record are so101_proximity_core.hpp's.  The pass is
// load_state, the columns of `q` (qpos[C.adr[k]] = q[i][k]: the addresses are kernel arguments, picked by a select over the lane index), kinematics.
// No dynamics runs and nothing is stored to a bound buffer.
//   * Bounding spheres of all geoms go into L.aabb (TGEOM columns), from the pose load_geom_at() gives with the body's xpos / xmat, as collision()
//     and k_tree_render_frames take it (this engine's geom_dyn is the body id).
//   * Groups are 256-bit masks held in eight registers each; membership is a select over the eight words, not an indexed array.
//   * The candidate list (pair word, bound) lives in the contact slots L.con, PROX_ROUND pairs per round: in the 32-dof build 64 contacts x 128 B is
//     exactly 2 x 1024 words.  The Dining scenes' 23 016 pairs are 23 rounds; the pair words are read four blocks of 64 in flight, the way
//     tree::broadphase reads them (one block per trip paid a round trip to the pair list each), and the ballots run block by block, so the list
//     stays in pair order.
//   * Members are appended in pair order, the smallest bound goes first, the walk stops when no bound is below the best, ties go to the earlier
//     pair, "geom1 in a" is tried before the swapped order: k_proximity's rules.
//   * A separated pair is the shared GJK with NoCache (hulls here go up to 5 676 vertices).  A pair whose simplex holds the origin or whose gap is
//     below PROX_HANDOVER goes to narrow_pair<HullCache, G64> on geoms loaded exactly as tree::collision() loads them: the reported distance is
//     what so101_tree_contacts reports as pair_dist, bit for bit.
static_assert(2 * PROX_ROUND * 4 <= sizeof(((TreeLDS*)0)->con), "the candidate list must fit the contact slots");
static_assert(PROX_ROUND % (4 * WAVE) == 0, "a round is a whole number of trips of four blocks");

// bit g of a 256-bit group mask held in eight registers (selects with constant indices: no scratch memory)
DEV bool tree_prox_member(unsigned int w0, unsigned int w1, unsigned int w2, unsigned int w3, unsigned int w4, unsigned int w5, unsigned int w6, unsigned int w7, int g) {
  const int k = (g >> 5) & 7;
  const unsigned int lo = k == 0 ? w0 : k == 1 ? w1 : k == 2 ? w2 : w3, hi = k == 4 ? w4 : k == 5 ? w5 : k == 6 ? w6 : w7;
  return (((k < 4 ? lo : hi) >> (g & 31)) & 1u) != 0u;
}

__global__ void __launch_bounds__(64) k_tree_proximity(const TreeModel* tm, const DevModel* gm, TreeBuffers B, int N, const int* env_index, const float* q, ProxCols C,
                                                       TouchPairsT<8> T, float max_dist, ProxOut O) {
  BLOCK_SHARED(TreeLDS, L);
  const int lane = wave_lane();
  const unsigned int npair_q = (unsigned int)T.npair;
  const size_t i = blockIdx.x / npair_q;
  const int p = wave_uniform_i((int)(blockIdx.x - (unsigned int)i * npair_q));
  const size_t o = (size_t)blockIdx.x;
  const int e = env_index ? wave_uniform_i(env_index[i]) : (int)i;
  const float zero[3] = {0.f, 0.f, 0.f};
  if (e < 0 || e >= N) { prox_store(o, max_dist, false, -1, -1, zero, zero, zero, max_dist, PROX_FLAG_OUTSIDE, 0, O); return; }
  tree::load_state(tm, L, B, e, N);
  if (q) {
    int adr = 0;
#pragma unroll
    for (int k = 0; k < PROX_MAXCOL; k++) adr = lane == k ? C.adr[k] : adr;
    if (lane < C.ncol) L.qpos[adr] = q[i * (size_t)C.ncol + lane];
    wave_sync();
  }
  tree::kinematics(tm, L);
  // bounding spheres: rows 0-2 the centre, row 3 the radius; a plane keeps its point in rows 0-2 and its normal in rows 3-5 (prox_bound)
  const int ngeom = ldc(&gm->ngeom);
  for (int g = lane; g < ngeom && g < TGEOM; g += WAVE) {
    int b = gm->geom_dyn[g];
    b = b < 0 ? 0 : b;
    GeomW G;
    load_geom_at<G16>(gm, g, L.xpos[b], L.xmat[b], G);
    const bool plane = G.type == G_PLANE;
#pragma unroll
    for (int k = 0; k < 3; k++) L.aabb[k][g] = plane ? G.p[k] : G.c[k];
    L.aabb[3][g] = plane ? G.R[2] : gm->geom_rbound[g];
    L.aabb[4][g] = plane ? G.R[5] : 0.f;
    L.aabb[5][g] = plane ? G.R[8] : 0.f;
  }
  wave_sync();
  const unsigned int a0 = T.a[p][0], a1 = T.a[p][1], a2 = T.a[p][2], a3 = T.a[p][3], a4 = T.a[p][4], a5 = T.a[p][5], a6 = T.a[p][6], a7 = T.a[p][7];
  const unsigned int b0 = T.b[p][0], b1 = T.b[p][1], b2 = T.b[p][2], b3 = T.b[p][3], b4 = T.b[p][4], b5 = T.b[p][5], b6 = T.b[p][6], b7 = T.b[p][7];
  unsigned int* cword = (unsigned int*)&L.con[0];
  float* cbound = (float*)&L.con[0] + PROX_ROUND;
  const unsigned int* pairs = ldc(&gm->pair_packed);
  const int npair = ldc(&gm->npair);
  float best = max_dist;
  bool found = false;
  int bg1 = -1, bg2 = -1, bflags = 0, bswap = 0, bround = 0, bidx = 0, queries = 0;
  float bpa[3] = {0.f, 0.f, 0.f}, bpb[3] = {0.f, 0.f, 0.f}, bn[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
  for (int c0 = 0; c0 < npair; c0 += PROX_ROUND) {
    // ---- the round's members and their bounds, appended in pair order
    int ncand = 0;
    wave_sync();                                         // (the previous round's list has been read)
#pragma unroll 1
    for (int j0 = 0; j0 < PROX_ROUND; j0 += 4 * WAVE) {
      if (c0 + j0 >= npair) break;
      unsigned int pk[4];
#pragma unroll
      for (int u = 0; u < 4; u++) { const int pi = c0 + j0 + u * WAVE + lane; pk[u] = pi < npair ? pairs[pi] : 0xffffffffu; }
      bool member[4], swapped[4];
      float lb[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const unsigned int w = pk[u];
        const bool valid = w != 0xffffffffu;
        int g1 = valid ? (int)(w & 0xffu) : 0, g2 = valid ? (int)((w >> 8) & 0xffu) : 0;
        g1 = g1 < TGEOM ? g1 : 0; g2 = g2 < TGEOM ? g2 : 0;
        const bool ab = tree_prox_member(a0, a1, a2, a3, a4, a5, a6, a7, g1) && tree_prox_member(b0, b1, b2, b3, b4, b5, b6, b7, g2);
        const bool ba = !ab && tree_prox_member(a0, a1, a2, a3, a4, a5, a6, a7, g2) && tree_prox_member(b0, b1, b2, b3, b4, b5, b6, b7, g1);
        lb[u] = prox_bound(L, w, g1, g2);
        member[u] = valid && (ab || ba) && lb[u] < max_dist;          // (a NaN bound: not a member)
        swapped[u] = ba;
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const unsigned long long mask = wave_ballot(member[u]);
        const int idx = ncand + wave_prefix(mask);
        if (member[u]) { cword[idx] = (pk[u] & 0x1ffffu) | (swapped[u] ? 0x20000u : 0u); cbound[idx] = lb[u]; }
        ncand += __popcll(mask);
      }
    }
    wave_sync();
    // ---- smallest bound first, until no bound is below the best
#pragma unroll 1
    for (int t = 0; t < PROX_ROUND; t++) {
      float val = -3.0e38f; int idx = 0x7fffffff;
      for (int k = lane; k < ncand; k += WAVE) { const float b = -cbound[k]; if (b > val) { val = b; idx = k; } }
      wave_argmax(val, idx);
      const float lbmin = -val;
      if (idx < 0 || idx >= ncand || !(lbmin <= best) || !(lbmin < max_dist)) break;
      const unsigned int w = cword[idx];
      wave_sync();
      if (lane == 0) cbound[idx] = 3.0e38f;
      wave_sync();
      const int g1 = wave_uniform_i((int)(w & 0xffu)), g2 = wave_uniform_i((int)((w >> 8) & 0xffu));
      const int bd1 = wave_uniform_i(tm->geom_body[g1]), bd2 = wave_uniform_i(tm->geom_body[g2]);
      GeomW G1, G2;
      load_geom_at(gm, g1, L.xpos[bd1], L.xmat[bd1], G1); load_geom_at(gm, g2, L.xpos[bd2], L.xmat[bd2], G2);
      ProxResult R;
      queries++;
      if (!prox_pair_geoms<HullCache, G64>(gm, G1, G2, g1, g2, best, R)) continue;
      // ties go to the earlier pair: within a round the list is in pair order, rounds come in pair order
      const bool better = R.dist < best || (found && R.dist == best && c0 == bround && idx < bidx);
      if (R.dist < max_dist && better) {
        best = R.dist; found = true; bg1 = g1; bg2 = g2; bflags = R.flags; bswap = (int)((w >> 17) & 1u); bround = c0; bidx = idx;
#pragma unroll
        for (int k = 0; k < 3; k++) { bpa[k] = R.pa[k]; bpb[k] = R.pb[k]; bn[k] = R.n[k]; }
      }
    }
  }
  // the a-side geom first: a member in the second order is reported swapped, its normal negated
  const bool sw = bswap != 0;
  const float na[3] = {sw ? -bn[0] : bn[0], sw ? -bn[1] : bn[1], sw ? -bn[2] : bn[2]};
  const float qa[3] = {sw ? bpb[0] : bpa[0], sw ? bpb[1] : bpa[1], sw ? bpb[2] : bpa[2]}, qb[3] = {sw ? bpa[0] : bpb[0], sw ? bpa[1] : bpb[1], sw ? bpa[2] : bpb[2]};
  prox_store(o, max_dist, found, sw ? bg2 : bg1, sw ? bg1 : bg2, qa, qb, na, best, bflags, queries, O);
}
}  // namespace TREE_NS
