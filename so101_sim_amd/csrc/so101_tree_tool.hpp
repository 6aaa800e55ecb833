// Cartesian tool control of the general-tree engine (so101_tree_tool_pose / so101_tree_tool_ik of include/so101.h): the pose of a frame fixed to an
// articulated body, its 6 x ncol Jacobian (MuJoCo's mj_jacSite: rows 0-2 jacp, rows 3-5 jacr) and a damped least-squares inverse kinematics solve,
// batched over entries.  Compiled once per build of the engine (tu_tree.hip, tu_tree64.hip), inside that build's namespace.
//
// Mapping: lane = entry, 64 entries per wavefront, as in so101_tool.hpp - not this engine's wavefront-per-env TreeLDS mapping.  A call works on one
// serial chain of at most 8 joints and one 6 x 6 solve: nothing 64 lanes could share, so every lane carries a whole entry in registers.
//
// The chain is computed on the host, once per call (tree_tool_chain in tu_tree.hip): the bodies between the world and the tool's body that carry a
// hinge or slide joint, root first; the jointless bodies between them folded in double precision into the fixed transform in front of the next
// joint, what lies below the last joint folded into the tool's own frame.  It arrives by value in the kernel-argument segment (wave-uniform
// scalar loads).  Loops over columns are unrolled to TREE_TOOL_MAXCOL with `k < ncol` as a wave-uniform branch, so every per-lane array is
// indexed by constants and lives in registers: no LDS, no scratch (scripts/kernel_resources.py).
//
// Per column the expressions of tree::kinematics() (so101_tree.hpp): xp += R pos, xq = xq * quat, hinge: xq = xq * (cos q/2, axis sin q/2),
// normquat, slide: xp += rot(axis, xq) * q.
#include "so101_tool_common.hpp"

#ifndef TREE_TOOL_MAXCOL
#define TREE_TOOL_MAXCOL 8
#endif

namespace TREE_NS {

// one column per joint of the chain, root first: the fixed transform from the previous column's body frame (the world for column 0) to this
// joint's body frame at q = 0, the joint axis in that frame, TJ_HINGE or TJ_SLIDE, and where its value sits in qpos; then the tool in the frame
// of the last column's body
struct TreeToolArg {
  int ncol;
  float pos[TREE_TOOL_MAXCOL][3], quat[TREE_TOOL_MAXCOL][4], axis[TREE_TOOL_MAXCOL][3];
  int type[TREE_TOOL_MAXCOL], qposadr[TREE_TOOL_MAXCOL];
  float tpos[3], tmat[9];
};
struct TreeIkArg { int mode, max_iters; float tol_pos, tol_rot, rot_weight, damping, max_step; unsigned int free_mask; float q_lo[TREE_TOOL_MAXCOL], q_hi[TREE_TOOL_MAXCOL]; };

// ---------------------------------------------------------------------------------------------------- forward kinematics of one entry
// q[ncol] -> tool position p, orientation M (row-major) and, with JAC, the Jacobian columns: hinge Jp[k] = a_k x (p - o_k), Jr[k] = a_k; slide
// Jp[k] = a_k, Jr[k] = 0 (a_k the world axis of joint k, o_k the world origin of its body: the joints sit at their body's origin); zero for k >= ncol.
template <bool JAC>
DEV void tree_tool_fk(const TreeToolArg& T, const float* q, float* p, float* M, float (*Jp)[3], float (*Jr)[3]) {
  const int ncol = T.ncol;
  float xp[3] = {0.f, 0.f, 0.f}, xq[4] = {1.f, 0.f, 0.f, 0.f};
  float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  float o[TREE_TOOL_MAXCOL][3], a[TREE_TOOL_MAXCOL][3];
#pragma unroll
  for (int k = 0; k < TREE_TOOL_MAXCOL; k++) {
#pragma unroll
    for (int i = 0; i < 3; i++) { o[k][i] = 0.f; a[k][i] = 0.f; }
  }
#pragma unroll
  for (int k = 0; k < TREE_TOOL_MAXCOL; k++) {
    if (k < ncol) {                     // wave-uniform: a scalar branch
      const float bp[3] = {T.pos[k][0], T.pos[k][1], T.pos[k][2]};
      const float bq[4] = {T.quat[k][0], T.quat[k][1], T.quat[k][2], T.quat[k][3]};
      const float ax[3] = {T.axis[k][0], T.axis[k][1], T.axis[k][2]};
      float t[3]; matvec3(t, R, bp);
      xp[0] += t[0]; xp[1] += t[1]; xp[2] += t[2];
      mulquat(xq, xq, bq);
      if (T.type[k] == TJ_HINGE) {
        float sn, cs; sincos_f(0.5f * q[k], &sn, &cs);
        float jq[4] = {cs, ax[0] * sn, ax[1] * sn, ax[2] * sn};
        mulquat(xq, xq, jq);
      }
      normquat(xq);
      if (T.type[k] == TJ_SLIDE) {
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
    for (int k = 0; k < TREE_TOOL_MAXCOL; k++) {
      const bool on = k < ncol, hinge = on && T.type[k] == TJ_HINGE;      // (wave-uniform; the selects keep -0 out of the columns that do not exist)
      float d[3] = {p[0] - o[k][0], p[1] - o[k][1], p[2] - o[k][2]};
      float c[3]; cross3(c, a[k], d);
#pragma unroll
      for (int i = 0; i < 3; i++) { Jp[k][i] = hinge ? c[i] : (on ? a[k][i] : 0.f); Jr[k][i] = hinge ? a[k][i] : 0.f; }
    }
  }
}

// where lane `i` of the call reads its joints: `q` [n][ncol] row-major when given, else the bound qpos [nq][n_envs] of env env_index[i] (or i) at the
// chain's qpos addresses.  Columns k >= ncol are 0.
DEV bool tree_tool_load_q(const TreeToolArg& T, const float* q, const float* qpos, int n_envs, const int* env_index, int i, float* out) {
  const int ncol = T.ncol;
  int e = 0;
  bool ok = true;
  if (!q) {
    e = env_index ? env_index[i] : i;
    ok = e >= 0 && e < n_envs;
  }
#pragma unroll
  for (int k = 0; k < TREE_TOOL_MAXCOL; k++) {
    out[k] = 0.f;
    if (k < ncol) {
      if (q) out[k] = q[(size_t)i * ncol + k];
      else if (ok) out[k] = qpos[(size_t)T.qposadr[k] * n_envs + e];
    }
  }
  return ok;
}

// ---------------------------------------------------------------------------------------------------- pose and Jacobian
// One lane per entry i < n.  An env_index entry outside [0, n_envs) reads nothing and gives NaN outputs.  jac [n][6][ncol] row-major: row r, column k.
__global__ void __launch_bounds__(64) k_tree_tool_pose(TreeToolArg T, const float* q, const float* qpos, int n_envs, const int* env_index, int n,
                                                       float* pos, float* mat, float* jac) {
  const int i = blockIdx.x * WAVE + wave_lane();
  if (i >= n) return;
  const int ncol = T.ncol;
  float qj[TREE_TOOL_MAXCOL];
  const bool ok = tree_tool_load_q(T, q, qpos, n_envs, env_index, i, qj);
  float p[3], M[9], Jp[TREE_TOOL_MAXCOL][3], Jr[TREE_TOOL_MAXCOL][3];
  if (jac) tree_tool_fk<true>(T, qj, p, M, Jp, Jr);
  else tree_tool_fk<false>(T, qj, p, M, Jp, Jr);
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
    float* J = jac + (size_t)i * 6 * ncol;
#pragma unroll
    for (int k = 0; k < TREE_TOOL_MAXCOL; k++) {
      if (k < ncol) {
#pragma unroll
        for (int r = 0; r < 3; r++) {
          J[r * ncol + k] = ok ? Jp[k][r] : nan;
          J[(r + 3) * ncol + k] = ok ? Jr[k][r] : nan;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------- inverse kinematics
// One lane per entry i < n; the algorithm is the one written down in include/so101.h for so101_tool_ik, over ncol columns, with a free_mask: a
// column whose bit is clear is zero in Jw and its joint keeps clamp(q_init).  Every lane iterates on its own values; a lane that has converged or
// used its iterations is frozen (its q, residual and info no longer change), and the loop ends when a ballot finds no lane running.  What a lane
// computes depends on its own inputs, the tool and the settings only - not on its neighbours in the wavefront, and not on n: a frozen lane runs the
// arithmetic of further rounds on its unchanged q and discards it.
__global__ void __launch_bounds__(64) k_tree_tool_ik(TreeToolArg T, TreeIkArg C, const float* target_pos, const float* target_mat, const float* q_init,
                                                     const float* qpos, int n_envs, const int* env_index, int n, float* q_out, float* residual, int* info) {
  const int i = blockIdx.x * WAVE + wave_lane();
  const bool in = i < n;               // (lanes past n stay in the loop's ballot: they are never active)
  const int ii = in ? i : 0;
  const int ncol = T.ncol;
  float q[TREE_TOOL_MAXCOL];
  const bool ok = tree_tool_load_q(T, q_init, qpos, n_envs, env_index, ii, q);
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
  for (int k = 0; k < TREE_TOOL_MAXCOL; k++) {
    if (k < ncol) q[k] = tool_clamp(q[k], C.q_lo[k], C.q_hi[k]);
  }
  bool active = in && ok && finite;
  int result = -1;
  float res_p = 0.f, res_r = 0.f;
  for (int it = 0;; it++) {
    float p[3], M[9], Jp[TREE_TOOL_MAXCOL][3], Jr[TREE_TOOL_MAXCOL][3];
    tree_tool_fk<true>(T, q, p, M, Jp, Jr);
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
    for (int k = 0; k < TREE_TOOL_MAXCOL; k++) {
      if (!((C.free_mask >> k) & 1u)) {                    // a held joint: no column (wave-uniform)
#pragma unroll
        for (int r = 0; r < 3; r++) { Jp[k][r] = 0.f; Jr[k][r] = 0.f; }
      }
    }
    float dq[TREE_TOOL_MAXCOL];
    tool_dls_step<TREE_TOOL_MAXCOL>(C.mode, C.rot_weight, C.damping, M, Jp, Jr, ep, er, dq);
    float big = 0.f;
#pragma unroll
    for (int k = 0; k < TREE_TOOL_MAXCOL; k++) big = fmaxf(big, fabsf(dq[k]));
    const float scale = big > C.max_step ? C.max_step / big : 1.f;
    if (active) {
#pragma unroll
      for (int k = 0; k < TREE_TOOL_MAXCOL; k++) {
        if ((C.free_mask >> k) & 1u) q[k] = tool_clamp(q[k] + dq[k] * scale, C.q_lo[k], C.q_hi[k]);
      }
    }
  }
  if (!in) return;
  const float nan = __int_as_float(0x7fc00000);
#pragma unroll
  for (int k = 0; k < TREE_TOOL_MAXCOL; k++) {
    if (k < ncol) q_out[(size_t)i * ncol + k] = ok ? q[k] : nan;
  }
  if (residual) { residual[(size_t)i * 2] = ok ? res_p : nan; residual[(size_t)i * 2 + 1] = ok ? res_r : nan; }
  if (info) info[i] = result;
}

}  // namespace TREE_NS
