// Contact sensing (so101_contacts of include/so101.h): the contact list of an env's CURRENT bound state and its reduction over pairs of geom
// groups, one wavefront per reported env.  The pass is MuJoCo's mj_forward cut down to what the report needs: load_state, kinematics and
// collision for the geometry; with `forces` also crba_arm, smooth_dynamics, make_constraints and the configured solver, with the iterations,
// tolerance and warmstart k_debug_forward uses.  Nothing is stored back - no bound buffer changes, the warmstart included.
//
// Where the numbers come from (read in the code, and checked bit for bit against the stage dump by the tests):
//   * Contact::frame is the FULL frame: contact_init() (so101_device.hpp) puts the normal (geom1 -> geom2) into row 0 and make_frame()
//     completes rows 1 and 2, MuJoCo's contact.frame.  The stage dump only shows row 0.
//   * Contact::f after the solve is the contact's force in that frame, what mj_contactForce returns and what DBG_FORCE dumps: solve_newton()
//     and solve_pgs() write all six entries on leaving, the ones beyond the contact's dim as zeros.  Before the solve the field holds the
//     mixed solimp (contact_init) - which is why `force` and the force sums need forces != 0 and are never written without it.
//   * L.overflow after the pass is diag word 4 of THIS pass: 1 candidate overflow, 2 contact overflow, 128 reduced to one contact per pair
//     from collision(); with forces the solve's bits as well (PGS: 2 when it drops the contacts beyond its 32).
//
// Lane = contact: MAXCON is 64, one wavefront.  The per-contact arrays are written element by element in the ABI's order ([n][C][k], element
// j * 64 + lane on pass j), so every store instruction of the wave covers 64 consecutive dwords whatever k is.  The touch part keeps each
// lane's own contact in registers, tests its two geoms against the pair's bitmasks (kernel arguments, like the tool chain) and reduces with
// the primitives of wave.hpp; the loop over the pairs is wave-uniform.  No atomics, no LDS round trip.
#pragma once
#include "so101_env.hpp"

DEV bool touch_member(const unsigned int* mask, int g) { return g >= 0 && ((mask[(g >> 5) & 3] >> (g & 31)) & 1u) != 0u; }

// K floats per contact of entry i, element j * 64 + lane per pass; `src` = offset of the field inside Contact (words); slots >= ncon get `fill`
template <int K>
DEV void store_contact_field(float* out, size_t i, const EnvLDS& L, int src, int ncon, float fill) {
  if (!out) return;
  int lane = wave_lane();
  float* o = out + i * (size_t)(MAXCON * K);
#pragma unroll
  for (int j = 0; j < K; j++) {
    int idx = j * WAVE + lane, k = idx / K, c = idx - k * K;
    o[idx] = k < ncon ? ((const float*)&L.con[k])[src + c] : fill;
  }
}

// an entry whose env index lies outside the batch reads nothing (the convention of so101_tool_pose): count -1, geoms -1, the touch part's
// ints 0, every float NaN
DEV void contacts_outside(size_t i, int npair, const ContactOut& O) {
  int lane = wave_lane();
  const float nan = __builtin_nanf("");
  if (lane == 0) { if (O.count) O.count[i] = -1; if (O.flags) O.flags[i] = 0; }
  if (O.geom) { O.geom[(i * MAXCON) * 2 + lane] = -1; O.geom[(i * MAXCON) * 2 + WAVE + lane] = -1; }
  if (O.dist) O.dist[i * MAXCON + lane] = nan;
  if (O.pos) for (int j = 0; j < 3; j++) O.pos[i * (MAXCON * 3) + j * WAVE + lane] = nan;
  if (O.frame) for (int j = 0; j < 9; j++) O.frame[i * (MAXCON * 9) + j * WAVE + lane] = nan;
  if (O.force) for (int j = 0; j < 6; j++) O.force[i * (MAXCON * 6) + j * WAVE + lane] = nan;
  if (lane < npair) {
    size_t p = i * (size_t)npair + lane;
    if (O.pair_count) O.pair_count[p] = 0;
    if (O.pair_dist) O.pair_dist[p] = nan;
    if (O.pair_normal) O.pair_normal[p] = nan;
    if (O.pair_force) { O.pair_force[3 * p] = nan; O.pair_force[3 * p + 1] = nan; O.pair_force[3 * p + 2] = nan; }
  }
}

template <int SOLVER>
__global__ void __launch_bounds__(64) k_contacts(const DevModel* m, StepParams P, DevBuffers B, const int* env_index, int forces, TouchPairs T, ContactOut O) {
  __shared__ EnvLDS L;
  const size_t i = blockIdx.x;
  const int lane = wave_lane();
  const int e = env_index ? wave_uniform_i(env_index[i]) : (int)i;
  if (e < 0 || e >= P.n_envs) { contacts_outside(i, T.npair, O); return; }
  load_state(L, B, e, P.n_envs);
  kinematics(m, L);
  if (forces) {                     // (wave-uniform: a kernel argument)
    crba_arm(m, L);
    smooth_dynamics(m, L);
  }
  collision(m, L);
  if (forces) {
    make_constraints(m, L);
    if constexpr (SOLVER == 1) solve_newton(m, L, P.iterations, P.tolerance); else solve_pgs(m, L, P.iterations, P.tolerance);
  }
  wave_sync();
  const int ncon = L.ncon;
  if (lane == 0) { if (O.count) O.count[i] = ncon; if (O.flags) O.flags[i] = L.overflow; }
  // ---- per-contact arrays
  if (O.geom) {
#pragma unroll
    for (int j = 0; j < 2; j++) {
      int idx = j * WAVE + lane, k = idx >> 1;
      O.geom[(i * MAXCON) * 2 + idx] = k < ncon ? ((idx & 1) ? L.con[k].g2 : L.con[k].g1) : -1;
    }
  }
  store_contact_field<1>(O.dist, i, L, (int)(offsetof(Contact, dist) / 4), ncon, __builtin_inff());
  store_contact_field<3>(O.pos, i, L, (int)(offsetof(Contact, pos) / 4), ncon, 0.f);
  store_contact_field<9>(O.frame, i, L, (int)(offsetof(Contact, frame) / 4), ncon, 0.f);
  if (forces) store_contact_field<6>(O.force, i, L, (int)(offsetof(Contact, f) / 4), ncon, 0.f);
  // ---- touch: lane = contact, one wave reduction per quantity and pair
  const int npair = T.npair;
  if (npair == 0) return;
  const bool live = lane < ncon;
  int g1 = -1, g2 = -1;
  float dist = __builtin_inff(), fn = 0.f, fw[3] = {0.f, 0.f, 0.f};
  if (live) {
    const Contact& c = L.con[lane];
    g1 = c.g1; g2 = c.g2; dist = c.dist;
    if (forces) {
      fn = c.f[0];
#pragma unroll
      for (int k = 0; k < 3; k++) fw[k] = c.frame[k] * c.f[0] + c.frame[3 + k] * c.f[1] + c.frame[6 + k] * c.f[2];      // R^T f[0:3]: the force on geom2's body, world frame
    }
  }
  for (int p = 0; p < npair; p++) {
    // first order that holds: group A has geom1 (the force on A is -R^T f), otherwise group A has geom2 (+R^T f)
    const bool ab = touch_member(T.a[p], g1) && touch_member(T.b[p], g2);
    const bool ba = !ab && touch_member(T.a[p], g2) && touch_member(T.b[p], g1);
    const bool in = live && (ab || ba);
    const int cnt = __popcll(wave_ballot(in));
    const float dmin = -wave_max_f(in ? -dist : -__builtin_inff());
    const size_t q = i * (size_t)npair + p;
    if (lane == 0 && O.pair_count) O.pair_count[q] = cnt;
    if (lane == 1 && O.pair_dist) O.pair_dist[q] = dmin;
    if (forces) {
      const float sgn = ab ? -1.f : 1.f;
      const float sn = wave_sum_f(in ? fn : 0.f);
      const float sx = wave_sum_f(in ? sgn * fw[0] : 0.f), sy = wave_sum_f(in ? sgn * fw[1] : 0.f), sz = wave_sum_f(in ? sgn * fw[2] : 0.f);
      if (lane == 2 && O.pair_normal) O.pair_normal[q] = sn;
      if (O.pair_force) {
        if (lane == 3) O.pair_force[3 * q] = sx;
        if (lane == 4) O.pair_force[3 * q + 1] = sy;
        if (lane == 5) O.pair_force[3 * q + 2] = sz;
      }
    }
  }
}
