// Contact sensing, the report tail both engines share (so101_contacts and so101_tree_contacts of include/so101.h): what k_contacts (so101_contacts.hpp)
// and k_tree_contacts (so101_tree_kernels.hpp) do once their own physics pass has left an env's contact list in LDS - count and flags, the
// per-contact arrays, and the reduction over pairs of geom groups.  One wavefront per reported entry.  Templated on the capacity CAP (contacts per
// entry: 64, or 64 / 160 in the two builds of the general-tree engine) and on the words NW of a group mask (4 or 8); where a contact's record and
// force live is the engine's business, handed in as a view:
//
//   struct View {
//     static constexpr int DIST, POS, FRAME;   // word offsets of dist, pos[3] and frame[9] inside a contact record
//     int count, flags;                        // the reported count (contacts 0 .. count - 1 are live) and the flag word of this pass
//     int g1(int k), g2(int k);                // geoms of contact k
//     const float* words(int k);               // contact k's record as float words
//     float force(int k, int j);               // component j < 6 of contact k's force in its frame (called only with forces)
//   };
//
// The frame is the FULL frame (rows: normal geom1 -> geom2, tangent 1, tangent 2) and force(k, 0..2) the force in it, so R^T f[0:3] is the force
// on geom2's body in the world frame.
//
// Lane = contact, in ceil(CAP / 64) passes (one at 64, three at 160, the last half-full).  The per-contact arrays are written in the ABI's order over
// the entry's flattened row ([n][CAP][K]: element idx = lane, lane + 64, ... < CAP * K - the bound is the element count: CAP * K is no multiple of 64
// for K = 1 at 160), so every store instruction of the wave covers consecutive dwords whatever K is; at CAP = 64 that is K stores per field.  The
// touch part keeps each lane's contacts in registers, tests their geoms against the pair's bitmasks (kernel arguments, like the tool chain),
// accumulates the lane's own contacts first and reduces once per quantity with the primitives of wave.hpp; the loop over the pairs is wave-uniform.
// No atomics, no LDS round trip.  A lane's sums start at +0 and a contact outside the pair adds nothing, so a lane without a member contributes +0
// to the wave's sum - and so does a member whose term is -0 (0 + -0 = +0): a pair sum is -0 never.
#pragma once
#include "wave.hpp"
#include "so101_math.hpp"
#include "so101_model.hpp"

template <int NW>
struct TouchPairsT {               // so101_geom_pair (NW = 4) / so101_tree_geom_pair (8), npair of them: bit (g & 31) of word g >> 5: geom g belongs to the group
  int npair;
  unsigned int a[TOUCH_MAX_PAIRS][NW], b[TOUCH_MAX_PAIRS][NW];
};

template <int NW>
DEV bool touch_member(const unsigned int* mask, int g) { return g >= 0 && ((mask[(g >> 5) & (NW - 1)] >> (g & 31)) & 1u) != 0u; }

// The element loops of the report, idx = lane, lane + 64, ... < CAP * K: with one lane per contact (CAP = 64) every lane makes exactly K trips and
// the loop is unrolled into K stores; beyond that the trip count depends on the lane and it stays a loop.
template <int CAP, int K> constexpr int contact_unroll = CAP == WAVE ? K : 1;

template <int CAP, int K>
DEV void fill_contact_field(float* out, size_t i, float fill) {
  if (!out) return;
  float* o = out + i * (size_t)(CAP * K);
  for (int idx = wave_lane(); idx < CAP * K; idx += WAVE) o[idx] = fill;
}

// K floats per contact of entry i from word `src` of the contact's record; slots >= the count get `fill`
template <int CAP, int K, class View>
DEV void store_contact_field(float* out, size_t i, const View& V, int src, float fill) {
  if (!out) return;
  float* o = out + i * (size_t)(CAP * K);
  constexpr int U = contact_unroll<CAP, K>;
#pragma unroll U
  for (int idx = wave_lane(); idx < CAP * K; idx += WAVE) {
    int k = idx / K, c = idx - k * K;
    o[idx] = k < V.count ? V.words(k)[src + c] : fill;
  }
}

// an entry whose env index lies outside the batch reads nothing (the convention of so101_tool_pose): count -1, flags 0, geoms -1, the touch
// part's counts 0, every float NaN
template <int CAP>
DEV void contacts_outside(size_t i, int npair, const ContactOut& O) {
  int lane = wave_lane();
  const float nan = __builtin_nanf("");
  if (lane == 0) { if (O.count) O.count[i] = -1; if (O.flags) O.flags[i] = 0; }
  if (O.geom) for (int idx = lane; idx < CAP * 2; idx += WAVE) O.geom[i * (size_t)(CAP * 2) + idx] = -1;
  fill_contact_field<CAP, 1>(O.dist, i, nan);
  fill_contact_field<CAP, 3>(O.pos, i, nan);
  fill_contact_field<CAP, 9>(O.frame, i, nan);
  fill_contact_field<CAP, 6>(O.force, i, nan);
  if (lane < npair) {
    size_t p = i * (size_t)npair + lane;
    if (O.pair_count) O.pair_count[p] = 0;
    if (O.pair_dist) O.pair_dist[p] = nan;
    if (O.pair_normal) O.pair_normal[p] = nan;
    if (O.pair_force) { O.pair_force[3 * p] = nan; O.pair_force[3 * p + 1] = nan; O.pair_force[3 * p + 2] = nan; }
  }
}

// entry i of the call from the contact list behind `V`; called by the whole wavefront, after the wave_sync() that ends the physics pass.
// `forces` (wave-uniform): the pass solved for the forces - without it `force`, `pair_normal` and `pair_force` are never written.
template <int CAP, int NW, class View>
DEV void contact_report(size_t i, const View& V, bool forces, const TouchPairsT<NW>& T, const ContactOut& O) {
  constexpr int PASSES = (CAP + WAVE - 1) / WAVE;
  const int lane = wave_lane();
  const int ncon = V.count;
  if (lane == 0) { if (O.count) O.count[i] = ncon; if (O.flags) O.flags[i] = V.flags; }
  // ---- per-contact arrays
  if (O.geom) {
    constexpr int U = contact_unroll<CAP, 2>;
#pragma unroll U
    for (int idx = lane; idx < CAP * 2; idx += WAVE) {
      int k = idx >> 1;
      O.geom[i * (size_t)(CAP * 2) + idx] = k < ncon ? ((idx & 1) ? V.g2(k) : V.g1(k)) : -1;
    }
  }
  store_contact_field<CAP, 1>(O.dist, i, V, View::DIST, __builtin_inff());
  store_contact_field<CAP, 3>(O.pos, i, V, View::POS, 0.f);
  store_contact_field<CAP, 9>(O.frame, i, V, View::FRAME, 0.f);
  if (forces && O.force) {
    float* o = O.force + i * (size_t)(CAP * 6);
    constexpr int U = contact_unroll<CAP, 6>;
#pragma unroll U
    for (int idx = lane; idx < CAP * 6; idx += WAVE) {
      int k = idx / 6, j = idx - k * 6;
      o[idx] = k < ncon ? V.force(k, j) : 0.f;
    }
  }
  // ---- touch: lane = contact (PASSES of them per lane), one wave reduction per quantity and pair
  const int npair = T.npair;
  if (npair == 0) return;
  int g1[PASSES], g2[PASSES];
  float dist[PASSES], fn[PASSES], fw[PASSES][3];
#pragma unroll
  for (int q = 0; q < PASSES; q++) {
    const int k = q * WAVE + lane;
    g1[q] = -1; g2[q] = -1; dist[q] = __builtin_inff(); fn[q] = 0.f; fw[q][0] = fw[q][1] = fw[q][2] = 0.f;
    if (k < ncon) {
      const float* c = V.words(k);
      g1[q] = V.g1(k); g2[q] = V.g2(k); dist[q] = c[View::DIST];
      if (forces) {
        const float f0 = V.force(k, 0), f1 = V.force(k, 1), f2 = V.force(k, 2);
        fn[q] = f0;
#pragma unroll
        for (int j = 0; j < 3; j++) fw[q][j] = c[View::FRAME + j] * f0 + c[View::FRAME + 3 + j] * f1 + c[View::FRAME + 6 + j] * f2;      // R^T f[0:3]: the force on geom2's body, world frame
      }
    }
  }
  for (int p = 0; p < npair; p++) {
    int cnt = 0;
    float dmin = __builtin_inff(), sn = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
    for (int q = 0; q < PASSES; q++) {
      // first order that holds: group A has geom1 (the force on A is -R^T f), otherwise group A has geom2 (+R^T f); a slot beyond count has geoms -1
      const bool ab = touch_member<NW>(T.a[p], g1[q]) && touch_member<NW>(T.b[p], g2[q]);
      const bool ba = !ab && touch_member<NW>(T.a[p], g2[q]) && touch_member<NW>(T.b[p], g1[q]);
      const bool in = ab || ba;
      cnt += __popcll(wave_ballot(in));
      if (in) {
        const float sgn = ab ? -1.f : 1.f;
        dmin = fminf(dmin, dist[q]);
        sn += fn[q]; sx += sgn * fw[q][0]; sy += sgn * fw[q][1]; sz += sgn * fw[q][2];
      }
    }
    dmin = -wave_max_f(-dmin);
    const size_t q = i * (size_t)npair + p;
    if (lane == 0 && O.pair_count) O.pair_count[q] = cnt;
    if (lane == 1 && O.pair_dist) O.pair_dist[q] = dmin;
    if (forces) {
      sn = wave_sum_f(sn); sx = wave_sum_f(sx); sy = wave_sum_f(sy); sz = wave_sum_f(sz);
      if (lane == 2 && O.pair_normal) O.pair_normal[q] = sn;
      if (O.pair_force) {
        if (lane == 3) O.pair_force[3 * q] = sx;
        if (lane == 4) O.pair_force[3 * q + 1] = sy;
        if (lane == 5) O.pair_force[3 * q + 2] = sz;
      }
    }
  }
}
