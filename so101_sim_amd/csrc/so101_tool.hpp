// Cartesian tool control of the SO100 engine (so101_tool_pose / so101_tool_ik of include/so101.h): the pose of a frame fixed to an arm link, its
// 6 x 6 Jacobian (MuJoCo's mj_jacSite: rows 0-2 jacp, rows 3-5 jacr) and a damped least-squares inverse kinematics solve, batched over envs.
//
// Mapping: lane = env, 64 envs per wavefront - unlike the step kernels, where a wavefront is one env.  The work of an env is a serial chain of six
// links and one 6 x 6 solve: nothing 64 lanes could share, so every lane carries a whole env in registers.  The model constants arrive through ldc
// (wave-uniform addresses: scalar loads), the tool and the solver settings through the kernel-argument segment (scalar loads as well).  Every
// per-lane array is indexed by constants after unrolling, so it lives in registers: no LDS, no scratch (scripts/kernel_resources.py).
//
// The chain is walked with the expressions of kinematics() (so101_device.hpp): quaternion product, normquat, quat2mat.
#pragma once
#include "so101_env.hpp"
#include "so101_tool_common.hpp"

// ---------------------------------------------------------------------------------------------------- forward kinematics of one env
// q[6] -> tool position p = xpos_b + R_b pos, orientation M = R_b mat (row-major) and, with JAC, the Jacobian columns: Jp[j] = a_j x (p - o_j),
// Jr[j] = a_j for j <= body (a_j the world axis of joint j, o_j the world origin of arm link j: the joints sit at their body's origin), zero beyond.
template <bool JAC>
DEV void tool_fk(const DevModel* m, const ToolArg& T, const float* q, float* p, float* M, float (*Jp)[3], float (*Jr)[3]) {
  const int body = T.body;
  float xp[3] = {ldc(&m->base_pos[0]), ldc(&m->base_pos[1]), ldc(&m->base_pos[2])};
  float xq[4] = {ldc(&m->base_quat[0]), ldc(&m->base_quat[1]), ldc(&m->base_quat[2]), ldc(&m->base_quat[3])};
  float R[9]; quat2mat(R, xq);
  float o[NARM][3], a[NARM][3];
#pragma unroll
  for (int k = 0; k < NARM; k++) {
#pragma unroll
    for (int i = 0; i < 3; i++) { o[k][i] = 0.f; a[k][i] = 0.f; }
  }
#pragma unroll
  for (int i = 0; i < 3; i++) p[i] = 0.f;
#pragma unroll
  for (int i = 0; i < 9; i++) M[i] = 0.f;
#pragma unroll
  for (int k = 0; k < NARM; k++) {
    if (k <= body) {                    // wave-uniform: a scalar branch
      const float ap[3] = {ldc(&m->arm_pos[k][0]), ldc(&m->arm_pos[k][1]), ldc(&m->arm_pos[k][2])};
      const float aq[4] = {ldc(&m->arm_quat[k][0]), ldc(&m->arm_quat[k][1]), ldc(&m->arm_quat[k][2]), ldc(&m->arm_quat[k][3])};
      const float ax[3] = {ldc(&m->arm_axis[k][0]), ldc(&m->arm_axis[k][1]), ldc(&m->arm_axis[k][2])};
      float t[3]; matvec3(t, R, ap);
      xp[0] += t[0]; xp[1] += t[1]; xp[2] += t[2];
      mulquat(xq, xq, aq);
      float sn, cs; sincos_f(0.5f * q[k], &sn, &cs);
      float jq[4] = {cs, ax[0] * sn, ax[1] * sn, ax[2] * sn};
      mulquat(xq, xq, jq);
      normquat(xq);
      quat2mat(R, xq);
      float wa[3]; matvec3(wa, R, ax);
#pragma unroll
      for (int i = 0; i < 3; i++) { o[k][i] = xp[i]; a[k][i] = wa[i]; }
      if (k == body) {
        const float tp[3] = {T.pos[0], T.pos[1], T.pos[2]};
        float tm[9];
#pragma unroll
        for (int i = 0; i < 9; i++) tm[i] = T.mat[i];
        float w[3]; matvec3(w, R, tp);
#pragma unroll
        for (int i = 0; i < 3; i++) p[i] = xp[i] + w[i];
        matmul3(M, R, tm);
      }
    }
  }
  if (JAC) {
#pragma unroll
    for (int j = 0; j < NARM; j++) {
      float d[3] = {p[0] - o[j][0], p[1] - o[j][1], p[2] - o[j][2]};
      float c[3]; cross3(c, a[j], d);
      const bool on = j <= body;       // (links beyond the tool's were never walked: their o and a are zero already; the select keeps -0 out)
#pragma unroll
      for (int i = 0; i < 3; i++) { Jp[j][i] = on ? c[i] : 0.f; Jr[j][i] = on ? a[j][i] : 0.f; }
    }
  }
}

// where lane `i` of the call reads its joints: `q` [n][6] row-major when given, else the bound qpos [nq][n_envs] of env env_index[i] (or i)
DEV bool tool_load_q(const float* q, const float* qpos, int n_envs, const int* env_index, int i, float* out) {
  if (q) {
#pragma unroll
    for (int j = 0; j < NARM; j++) out[j] = q[(size_t)i * NARM + j];
    return true;
  }
  const int e = env_index ? env_index[i] : i;
  const bool ok = e >= 0 && e < n_envs;
#pragma unroll
  for (int j = 0; j < NARM; j++) out[j] = ok ? qpos[(size_t)j * n_envs + e] : 0.f;
  return ok;
}

// ---------------------------------------------------------------------------------------------------- pose and Jacobian
// One lane per entry i < n.  An env_index entry outside [0, n_envs) reads nothing and gives NaN outputs.  jac [n][6][6] row-major: row r, column j.
__global__ void __launch_bounds__(64) k_tool_pose(const DevModel* m, ToolArg T, const float* q, const float* qpos, int n_envs, const int* env_index, int n,
                                                  float* pos, float* mat, float* jac) {
  const int i = blockIdx.x * WAVE + wave_lane();
  if (i >= n) return;
  float qj[NARM];
  const bool ok = tool_load_q(q, qpos, n_envs, env_index, i, qj);
  float p[3], M[9], Jp[NARM][3], Jr[NARM][3];
  if (jac) tool_fk<true>(m, T, qj, p, M, Jp, Jr);
  else tool_fk<false>(m, T, qj, p, M, Jp, Jr);
  const float nan = __int_as_float(0x7fc00000);
  if (pos) {
#pragma unroll
    for (int k = 0; k < 3; k++) pos[(size_t)i * 3 + k] = ok ? p[k] : nan;
  }
  if (mat) {
#pragma unroll
    for (int k = 0; k < 9; k++) mat[(size_t)i * 9 + k] = ok ? M[k] : nan;
  }
  if (jac) {
#pragma unroll
    for (int j = 0; j < NARM; j++) {
#pragma unroll
      for (int r = 0; r < 3; r++) {
        jac[(size_t)i * 36 + r * 6 + j] = ok ? Jp[j][r] : nan;
        jac[(size_t)i * 36 + (r + 3) * 6 + j] = ok ? Jr[j][r] : nan;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- inverse kinematics
// (tool_clamp, tool_rotvec, tool_rot_error and tool_dls_step<columns>: so101_tool_common.hpp)

// One lane per entry i < n; the algorithm is written down in include/so101.h (so101_tool_ik).  Every lane iterates on its own values; a lane that
// has converged or used its iterations is frozen (its q, residual and info no longer change), and the loop ends when a ballot finds no lane running.
// What a lane computes depends on its own inputs and the settings only - not on its neighbours in the wavefront, and not on n: a frozen lane runs
// the arithmetic of further rounds on its unchanged q and discards it.
__global__ void __launch_bounds__(64) k_tool_ik(const DevModel* m, ToolArg T, IkArg C, const float* target_pos, const float* target_mat, const float* q_init,
                                                const float* qpos, int n_envs, const int* env_index, int n, float* q_out, float* residual, int* info) {
  const int i = blockIdx.x * WAVE + wave_lane();
  const bool in = i < n;               // (lanes past n stay in the loop's ballot: they are never active)
  const int ii = in ? i : 0;
  float q[NARM];
  const bool ok = tool_load_q(q_init, qpos, n_envs, env_index, ii, q);
  float pt[3], Mt[9];
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 3; k++) { pt[k] = target_pos[(size_t)ii * 3 + k]; finite = finite && fabsf(pt[k]) <= 3.0e38f; }
#pragma unroll
  for (int k = 0; k < 9; k++) {
    Mt[k] = C.mode != 0 ? target_mat[(size_t)ii * 9 + k] : (k % 4 == 0 ? 1.f : 0.f);
    finite = finite && fabsf(Mt[k]) <= 3.0e38f;          // (false for NaN as well)
  }
#pragma unroll
  for (int j = 0; j < NARM; j++) q[j] = tool_clamp(q[j], C.q_lo[j], C.q_hi[j]);
  bool active = in && ok && finite;
  int result = -1;
  float res_p = 0.f, res_r = 0.f;
  for (int it = 0;; it++) {
    float p[3], M[9], Jp[NARM][3], Jr[NARM][3];
    tool_fk<true>(m, T, q, p, M, Jp, Jr);
    float ep[3] = {pt[0] - p[0], pt[1] - p[1], pt[2] - p[2]}, er[3];
    tool_rot_error(C.mode, M, Mt, er);
    const float np = sqrtf(dot3(ep, ep)), nr = sqrtf(dot3(er, er));
    if (active || it == 0) { res_p = np; res_r = nr; }
    if (active) {
      if (np <= C.tol_pos && nr <= C.tol_rot) { result = it; active = false; }
      else if (it >= C.max_iters) active = false;
    }
    if (!wave_ballot(active)) break;
    float dq[NARM];
    tool_dls_step<NARM>(C.mode, C.rot_weight, C.damping, M, Jp, Jr, ep, er, dq);
    float big = 0.f;
#pragma unroll
    for (int j = 0; j < NARM; j++) big = fmaxf(big, fabsf(dq[j]));
    const float scale = big > C.max_step ? C.max_step / big : 1.f;
    if (active) {
#pragma unroll
      for (int j = 0; j < NARM; j++) q[j] = tool_clamp(q[j] + dq[j] * scale, C.q_lo[j], C.q_hi[j]);
    }
  }
  if (!in) return;
  const float nan = __int_as_float(0x7fc00000);
#pragma unroll
  for (int j = 0; j < NARM; j++) q_out[(size_t)i * NARM + j] = ok ? q[j] : nan;
  if (residual) { residual[(size_t)i * 2] = ok ? res_p : nan; residual[(size_t)i * 2 + 1] = ok ? res_r : nan; }
  if (info) info[i] = result;
}
