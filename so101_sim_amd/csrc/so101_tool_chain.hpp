// Cartesian tool control of both engines (so101_tool_pose / so101_tool_ik and so101_tree_tool_pose / so101_tree_tool_ik of include/so101.h): the
// pose of a frame fixed to an articulated body, its 6 x nio Jacobian (MuJoCo's mj_jacSite: rows 0-2 jacp, rows 3-5 jacr) and a damped
// least-squares inverse kinematics solve, batched over entries.  One pair of kernels, templated on the column capacity NC: 6 for the SO100
// engine, 8 for the general-tree engine (both of its builds call the same instantiation).  Compiled in tu_misc.hip, launched through
// so101_launch.hpp.
//
// Mapping: lane = entry, 64 entries per wavefront - unlike the step kernels, where a wavefront is one env.  A call works on one serial chain of
// at most NC joints and one 6 x 6 solve: nothing 64 lanes could share, so every lane carries a whole entry in registers.
//
// The chain is built on the host, once per call, and arrives by value in the kernel-argument segment (wave-uniform scalar loads), as do the
// solver settings.  SO100: the base as the root, one hinge column per arm link up to the tool's (so101_hip.hip).  Tree: the bodies between the
// world and the tool's body that carry a hinge or slide joint, the jointless ones folded in double precision into the next column
// (tree_tool_chain in so101_tree_host.hpp).  Loops over columns are unrolled to NC with `k < ncol` / `k < nio` as wave-uniform branches, so every
// per-lane array is indexed by constants and lives in registers: no LDS, no scratch (scripts/kernel_resources.py).
//
// Per column the expressions of kinematics() (so101_device.hpp) and tree::kinematics() (so101_tree.hpp): xp += R pos, xq = xq * quat, hinge:
// xq = xq * (cos q/2, axis sin q/2), normquat, slide: xp += rot(axis, xq) * q, quat2mat.
#pragma once
#include "wave.hpp"
#include "so101_tool_common.hpp"

enum { TOOL_HINGE = 1, TOOL_SLIDE = 3 };      // column types: the values of TJ_HINGE / TJ_SLIDE (so101_tree.hpp) and of so101_tree_tool_chain's jnt_type

// The root transform (world to the frame the first column is given in; the quaternion is used as it is, not normalised), then one column per
// walked joint, root first: the fixed transform from the previous column's body frame (the root for column 0) to this joint's body frame at
// q = 0, the joint axis in that frame, its type, and where its value sits in qpos; then the tool in the frame of the last walked column's body.
// nio >= ncol is the row stride of q, q_init, q_out, jac and the limits: columns ncol <= k < nio (SO100 joints beyond the tool's link) are
// loaded, clamped and written back by the IK, never stepped, and their Jacobian columns are +0; only their qposadr is read.
template <int NC>
struct ToolChain {
  int ncol, nio;
  float rpos[3], rquat[4];
  float pos[NC][3], quat[NC][4], axis[NC][3];
  int type[NC], qposadr[NC];
  float tpos[3], tmat[9];
};
// The chain as k_tool_ik reads it: through the kernel-argument segment where it is used (constant address space: scalar loads that the compiler
// may repeat inside the IK loop) instead of the by-value parameter, all of which is loaded at entry and then kept in scalar registers across
// the loop - 324 (NC = 6) / 482 (NC = 8) of them spilled to VGPR lanes that way, 50 / 74 this way (profiles/README.md has the times).  The
// chain must be the kernel's FIRST parameter: the explicit arguments start at offset 0 of the segment.
template <int NC>
DEV const ToolChain<NC>& chain_argument(const ToolChain<NC>& by_value) {
#ifdef SO101_EMU
  return by_value;
#else
  (void)by_value;
  return *(const ToolChain<NC>*)__builtin_amdgcn_kernarg_segment_ptr();
#endif
}
// the solver settings of one IK call; free_mask bit k clear: column k is zero in Jw and its joint keeps clamp(q_init)
template <int NC>
struct IkSettings { int mode, max_iters; float tol_pos, tol_rot, rot_weight, damping, max_step; unsigned int free_mask; float q_lo[NC], q_hi[NC]; };

// ---------------------------------------------------------------------------------------------------- forward kinematics of one entry
// q[nio] -> tool position p, orientation M (row-major) and, with JAC, the Jacobian columns: hinge Jp[k] = a_k x (p - o_k), Jr[k] = a_k; slide
// Jp[k] = a_k, Jr[k] = 0 (a_k the world axis of joint k, o_k the world origin of its body: the joints sit at their body's origin); zero for k >= ncol.
template <int NC, bool JAC>
DEV void tool_fk(const ToolChain<NC>& T, const float* q, float* p, float* M, float (*Jp)[3], float (*Jr)[3]) {
  const int ncol = T.ncol;
  float xp[3] = {T.rpos[0], T.rpos[1], T.rpos[2]}, xq[4] = {T.rquat[0], T.rquat[1], T.rquat[2], T.rquat[3]};
  float R[9]; quat2mat(R, xq);
  float o[NC][3], a[NC][3];
#pragma unroll
  for (int k = 0; k < NC; k++) {
#pragma unroll
    for (int i = 0; i < 3; i++) { o[k][i] = 0.f; a[k][i] = 0.f; }
  }
#pragma unroll
  for (int k = 0; k < NC; k++) {
    if (k < ncol) {                     // wave-uniform: a scalar branch
      const float bp[3] = {T.pos[k][0], T.pos[k][1], T.pos[k][2]};
      const float bq[4] = {T.quat[k][0], T.quat[k][1], T.quat[k][2], T.quat[k][3]};
      const float ax[3] = {T.axis[k][0], T.axis[k][1], T.axis[k][2]};
      float t[3]; matvec3(t, R, bp);
      xp[0] += t[0]; xp[1] += t[1]; xp[2] += t[2];
      mulquat(xq, xq, bq);
      if (T.type[k] == TOOL_HINGE) {
        float sn, cs; sincos_f(0.5f * q[k], &sn, &cs);
        float jq[4] = {cs, ax[0] * sn, ax[1] * sn, ax[2] * sn};
        mulquat(xq, xq, jq);
      }
      normquat(xq);
      if (T.type[k] == TOOL_SLIDE) {
        float s[3]; rotvecquat(s, ax, xq);
        xp[0] += s[0] * q[k]; xp[1] += s[1] * q[k]; xp[2] += s[2] * q[k];
      }
      quat2mat(R, xq);
      float wa[3]; matvec3(wa, R, ax);
#pragma unroll
      for (int i = 0; i < 3; i++) { o[k][i] = xp[i]; a[k][i] = wa[i]; }
    }
  }
  {
    const float tp[3] = {T.tpos[0], T.tpos[1], T.tpos[2]};
    float tm[9];
#pragma unroll
    for (int i = 0; i < 9; i++) tm[i] = T.tmat[i];
    float w[3]; matvec3(w, R, tp);
#pragma unroll
    for (int i = 0; i < 3; i++) p[i] = xp[i] + w[i];
    matmul3(M, R, tm);
  }
  if (JAC) {
#pragma unroll
    for (int k = 0; k < NC; k++) {
      const bool on = k < ncol, hinge = on && T.type[k] == TOOL_HINGE;      // (wave-uniform; the selects keep -0 out of the columns that were not walked)
      float d[3] = {p[0] - o[k][0], p[1] - o[k][1], p[2] - o[k][2]};
      float c[3]; cross3(c, a[k], d);
#pragma unroll
      for (int i = 0; i < 3; i++) { Jp[k][i] = hinge ? c[i] : (on ? a[k][i] : 0.f); Jr[k][i] = hinge ? a[k][i] : 0.f; }
    }
  }
}

// where lane `i` of the call reads its joints: `q` [n][nio] row-major when given, else the bound qpos [nq][n_envs] of env env_index[i] (or i) at the
// chain's qpos addresses.  Columns k >= nio are 0.
template <int NC>
DEV bool tool_load_q(const ToolChain<NC>& T, const float* q, const float* qpos, int n_envs, const int* env_index, int i, float* out) {
  const int nio = T.nio;
  int e = 0;
  bool ok = true;
  if (!q) {
    e = env_index ? env_index[i] : i;
    ok = e >= 0 && e < n_envs;
  }
#pragma unroll
  for (int k = 0; k < NC; k++) {
    out[k] = 0.f;
    if (k < nio) {
      if (q) out[k] = q[(size_t)i * nio + k];
      else if (ok) out[k] = qpos[(size_t)T.qposadr[k] * n_envs + e];
    }
  }
  return ok;
}

// ---------------------------------------------------------------------------------------------------- pose and Jacobian
// One lane per entry i < n.  An env_index entry outside [0, n_envs) reads nothing and gives NaN outputs.  jac [n][6][nio] row-major: row r, column k.
template <int NC>
__global__ void __launch_bounds__(64) k_tool_pose(ToolChain<NC> T, const float* q, const float* qpos, int n_envs, const int* env_index, int n,
                                                  float* pos, float* mat, float* jac) {
  const int i = blockIdx.x * WAVE + wave_lane();
  if (i >= n) return;
  const int nio = T.nio;
  float qj[NC];
  const bool ok = tool_load_q<NC>(T, q, qpos, n_envs, env_index, i, qj);
  float p[3], M[9], Jp[NC][3], Jr[NC][3];
  if (jac) tool_fk<NC, true>(T, qj, p, M, Jp, Jr);
  else tool_fk<NC, false>(T, qj, p, M, Jp, Jr);
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
    float* J = jac + (size_t)i * 6 * nio;
#pragma unroll
    for (int k = 0; k < NC; k++) {
      if (k < nio) {
#pragma unroll
        for (int r = 0; r < 3; r++) {
          J[r * nio + k] = ok ? Jp[k][r] : nan;
          J[(r + 3) * nio + k] = ok ? Jr[k][r] : nan;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- inverse kinematics
// (tool_clamp, tool_rotvec, tool_rot_error and tool_dls_step<columns>: so101_tool_common.hpp)

// One lane per entry i < n; the algorithm is written down in include/so101.h (so101_tool_ik), here over ncol columns with a free_mask.  Every lane
// iterates on its own values; a lane that has converged or used its iterations is frozen (its q, residual and info no longer change), and the
// loop ends when a ballot finds no lane running.  What a lane computes depends on its own inputs, the tool and the settings only - not on its
// neighbours in the wavefront, and not on n: a frozen lane runs the arithmetic of further rounds on its unchanged q and discards it.
template <int NC>
__global__ void __launch_bounds__(64) k_tool_ik(ToolChain<NC> chain, IkSettings<NC> C, const float* target_pos, const float* target_mat, const float* q_init,
                                                const float* qpos, int n_envs, const int* env_index, int n, float* q_out, float* residual, int* info) {
  const ToolChain<NC>& T = chain_argument<NC>(chain);
  const int i = blockIdx.x * WAVE + wave_lane();
  const bool in = i < n;               // (lanes past n stay in the loop's ballot: they are never active)
  const int ii = in ? i : 0;
  const int ncol = T.ncol, nio = T.nio;
  float q[NC];
  const bool ok = tool_load_q<NC>(T, q_init, qpos, n_envs, env_index, ii, q);
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
  for (int k = 0; k < NC; k++) {
    if (k < nio) q[k] = tool_clamp(q[k], C.q_lo[k], C.q_hi[k]);
  }
  bool active = in && ok && finite;
  int result = -1;
  float res_p = 0.f, res_r = 0.f;
  for (int it = 0;; it++) {
    float p[3], M[9], Jp[NC][3], Jr[NC][3];
    tool_fk<NC, true>(T, q, p, M, Jp, Jr);
    float ep[3] = {pt[0] - p[0], pt[1] - p[1], pt[2] - p[2]}, er[3];
    tool_rot_error(C.mode, M, Mt, er);
    const float np = sqrtf(dot3(ep, ep)), nr = sqrtf(dot3(er, er));
    if (active || it == 0) { res_p = np; res_r = nr; }
    if (active) {
      if (np <= C.tol_pos && nr <= C.tol_rot) { result = it; active = false; }
      else if (it >= C.max_iters) active = false;
    }
    if (!wave_ballot(active)) break;
#pragma unroll
    for (int k = 0; k < NC; k++) {
      if (!((C.free_mask >> k) & 1u)) {                    // a held joint: no column (wave-uniform)
#pragma unroll
        for (int r = 0; r < 3; r++) { Jp[k][r] = 0.f; Jr[k][r] = 0.f; }
      }
    }
    float dq[NC];
    tool_dls_step<NC>(C.mode, C.rot_weight, C.damping, M, Jp, Jr, ep, er, dq);
    float big = 0.f;
#pragma unroll
    for (int k = 0; k < NC; k++) big = fmaxf(big, fabsf(dq[k]));
    const float scale = big > C.max_step ? C.max_step / big : 1.f;
    if (active) {
#pragma unroll
      for (int k = 0; k < NC; k++) {
        if (k < ncol && ((C.free_mask >> k) & 1u)) q[k] = tool_clamp(q[k] + dq[k] * scale, C.q_lo[k], C.q_hi[k]);
      }
    }
  }
  if (!in) return;
  const float nan = __int_as_float(0x7fc00000);
#pragma unroll
  for (int k = 0; k < NC; k++) {
    if (k < nio) q_out[(size_t)i * nio + k] = ok ? q[k] : nan;
  }
  if (residual) { residual[(size_t)i * 2] = ok ? res_p : nan; residual[(size_t)i * 2 + 1] = ok ? res_r : nan; }
  if (info) info[i] = result;
}
