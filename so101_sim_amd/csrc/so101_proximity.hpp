// Proximity sensing of the SO100 engine (so101_proximity of include/so101.h): k_proximity, one wavefront per (entry, group pair) - block b serves
// entry b / npair and pair b % npair.  The pass is load_state, the arm's joint angles from `q` when given, kinematics - no dynamics, no constraint
// code, and nothing is stored to a bound buffer.  How candidates are chosen and what the exact query is: so101_proximity_core.hpp, shared with the
// general-tree engine.  What is this engine's own: where a geom's pose comes from (load_geom), 128-bit groups, q as the six arm joints, and the
// fused step's narrowphase policy (NoCache, the whole wavefront on one pair) for the pairs that touch.
#pragma once
#include "so101_env.hpp"
#include "so101_contact_report.hpp"
#include "so101_proximity_core.hpp"

static_assert(2 * PROX_ROUND * 4 <= sizeof(((EnvLDS*)0)->con), "the candidate list must fit the contact slots");

// one admitted pair (geom types ordered, as in the pair list): false when the pair is farther than `cutoff`
DEV bool prox_pair(const DevModel* m, const EnvLDS& L, int g1, int g2, float cutoff, ProxResult& R) {
  GeomW G1, G2;
  load_geom(m, L, g1, G1); load_geom(m, L, g2, G2);
  return prox_pair_geoms<NoCache, G64>(m, G1, G2, g1, g2, cutoff, R);
}

// bounding spheres of all geoms in the world, into the geom-box slots of EnvLDS: rows 0-2 the centre, row 3 the radius; a plane keeps its
// point in rows 0-2 and its normal in rows 3-5 (the pair word says which geom is a plane)
DEV void prox_spheres(const DevModel* m, EnvLDS& L) {
  const int ngeom = ldc(&m->ngeom);
  for (int g = wave_lane(); g < ngeom && g < MAXGEOM; g += WAVE) {
    const float* gp = m->geom_pos + 3 * g; const float* gm = m->geom_mat + 9 * g; const float* gc = m->geom_center + 3 * g;
    const int d = m->geom_dyn[g];
    float R[9], p[3], lm[9], lp[3] = {gp[0], gp[1], gp[2]}, lc[3] = {gc[0], gc[1], gc[2]};
#pragma unroll
    for (int i = 0; i < 9; i++) lm[i] = gm[i];
    if (d < 0) {
#pragma unroll
      for (int i = 0; i < 9; i++) R[i] = lm[i];
#pragma unroll
      for (int i = 0; i < 3; i++) p[i] = lp[i];
    } else {
      matmul3(R, L.xmat[d], lm);
      float t[3]; matvec3(t, L.xmat[d], lp);
#pragma unroll
      for (int i = 0; i < 3; i++) p[i] = L.xpos[d][i] + t[i];
    }
    float cw[3]; matvec3(cw, R, lc);
    const bool plane = m->geom_type[g] == G_PLANE;
#pragma unroll
    for (int i = 0; i < 3; i++) L.aabb[i][g] = plane ? p[i] : p[i] + cw[i];
    L.aabb[3][g] = plane ? R[2] : m->geom_rbound[g];
    L.aabb[4][g] = plane ? R[5] : 0.f;
    L.aabb[5][g] = plane ? R[8] : 0.f;
  }
  wave_sync();
}

// bit g of a 128-bit group mask held in four registers (a select, not an indexed array: no scratch memory)
DEV bool prox_member(unsigned int w0, unsigned int w1, unsigned int w2, unsigned int w3, int g) {
  const int k = (g >> 5) & 3;
  const unsigned int w = k == 0 ? w0 : k == 1 ? w1 : k == 2 ? w2 : w3;
  return ((w >> (g & 31)) & 1u) != 0u;
}

__global__ void __launch_bounds__(64) k_proximity(const DevModel* m, StepParams P, DevBuffers B, const int* env_index, const float* q, TouchPairsT<4> T, float max_dist,
                                                  ProxOut O) {
  __shared__ EnvLDS L;
  const int lane = wave_lane();
  const unsigned int npair_q = (unsigned int)T.npair;
  const size_t i = blockIdx.x / npair_q;
  const int p = wave_uniform_i((int)(blockIdx.x - (unsigned int)i * npair_q));
  const size_t o = (size_t)blockIdx.x;
  const int e = env_index ? wave_uniform_i(env_index[i]) : (int)i;
  const float zero[3] = {0.f, 0.f, 0.f};
  if (e < 0 || e >= P.n_envs) { prox_store(o, max_dist, false, -1, -1, zero, zero, zero, max_dist, PROX_FLAG_OUTSIDE, 0, O); return; }
  load_state(L, B, e, P.n_envs);
  if (q) {
    if (lane < NARM) L.qpos[lane] = q[i * NARM + lane];
    wave_sync();
  }
  kinematics(m, L);
  prox_spheres(m, L);
  const unsigned int a0 = T.a[p][0], a1 = T.a[p][1], a2 = T.a[p][2], a3 = T.a[p][3], b0 = T.b[p][0], b1 = T.b[p][1], b2 = T.b[p][2], b3 = T.b[p][3];
  unsigned int* cword = (unsigned int*)&L.con[0];
  float* cbound = (float*)&L.con[0] + PROX_ROUND;
  const unsigned int* pairs = ldc(&m->pair_packed);
  const int npair = ldc(&m->npair);
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
    for (int j = 0; j < PROX_ROUND / WAVE; j++) {
      const int pi = c0 + j * WAVE + lane;
      if (c0 + j * WAVE >= npair) break;
      const unsigned int w = pi < npair ? pairs[pi] : 0xffffffffu;
      const bool valid = w != 0xffffffffu;
      int g1 = valid ? (int)(w & 0xffu) : 0, g2 = valid ? (int)((w >> 8) & 0xffu) : 0;
      g1 = g1 < MAXGEOM ? g1 : 0; g2 = g2 < MAXGEOM ? g2 : 0;
      const bool ab = prox_member(a0, a1, a2, a3, g1) && prox_member(b0, b1, b2, b3, g2);
      const bool ba = !ab && prox_member(a0, a1, a2, a3, g2) && prox_member(b0, b1, b2, b3, g1);
      const float lb = prox_bound(L, w, g1, g2);
      const bool member = valid && (ab || ba) && lb < max_dist;          // (a NaN bound: not a member)
      const unsigned long long mask = wave_ballot(member);
      const int idx = ncand + wave_prefix(mask);
      if (member) { cword[idx] = (w & 0x1ffffu) | (ba ? 0x20000u : 0u); cbound[idx] = lb; }
      ncand += __popcll(mask);
    }
    wave_sync();
    // ---- smallest bound first, until no bound is below the best
#pragma unroll 1
    for (int t = 0; t < PROX_ROUND; t++) {
      float val = -3.0e38f; int idx = 0x7fffffff;
      for (int k = lane; k < ncand; k += WAVE) { const float b = -cbound[k]; if (b > val) { val = b; idx = k; } }
      wave_argmax(val, idx);
      const float lb = -val;
      if (idx < 0 || idx >= ncand || !(lb <= best) || !(lb < max_dist)) break;
      const unsigned int w = cword[idx];
      wave_sync();
      if (lane == 0) cbound[idx] = 3.0e38f;
      wave_sync();
      const int g1 = (int)(w & 0xffu), g2 = (int)((w >> 8) & 0xffu);
      ProxResult R;
      queries++;
      if (!prox_pair(m, L, g1, g2, best, R)) continue;
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
