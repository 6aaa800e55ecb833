// Contact sensing of the general-tree engine (so101_tree_contacts of include/so101.h): the contact list of an env's CURRENT bound state and its
// reduction over pairs of geom groups, one wavefront per reported entry - so101_contacts.hpp on this engine's device functions.  Included once per
// build of the engine (TREE_VARIANT), behind so101_tree.hpp: no include guard.
//
// The pass is tree::forward() cut down to the report, its stages in forward()'s order - which is what makes the numbers bit-identical to
// k_tree_forward's dump: load_state, kinematics; with `forces` crba, rne_bias, smooth; collision; with `forces` make_constraints and
// solve_newton with the handle's iterations and tolerance.  `forces` is a kernel argument: the branch is wave-uniform, and without it none of
// the dynamics runs.  Nothing is stored back - no store_state, no store_diag, the warmstart is read and left alone.
//
// Where the numbers come from:
//   * TCon::frame is the FULL frame: write_contact() puts the normal (geom1 -> geom2) into row 0 and make_frame() completes rows 1 and 2.
//   * count and the per-contact geometry are those after collision(), read before make_constraints() runs: make_constraints() lowers L.ncon when
//     the rows of the last contacts do not fit TROW (flag 4).  Geometry with and without forces is therefore the same, bit for bit; the
//     contacts that got no rows report zero force and add nothing to the sums.
//   * force[j] = G.ef[c.row + j] for j < c.dim, zero beyond - read through the TreeScratch the solve used (use_row_storage() may have moved the
//     rows into LDS) - and only when the pass has rows at all (nrow > 0, as k_tree_forward's TDBG_FORCE): without rows solve_newton() returns
//     before anything writes ef.
//   * L.flags, started at 0, is the flag word of THIS pass: 1 candidate overflow, 2 contact overflow (collision() ends the list at the first
//     pair that does not fit), with forces 4 (contacts dropped for rows).
//
// Scratch: make_constraints() and solve_newton() work in a per-env slice of B.scratch.  env_index may name an env more than once, and two
// wavefronts on one slice would race: entry i works in slice i mod n_envs, and the host enqueues at most n_envs entries per launch
// (tu_tree.hip).  No kernel of this engine reads scratch it did not write in the same launch, so whose slice it is does not matter.
//
// Lane = contact, in ceil(TCON / 64) passes (one in the 32-dof build, three in the 64-dof build, the last half-full).  The per-contact arrays
// are written in the ABI's order over the entry's flattened row ([n][TCON][K]: element idx = lane, lane + 64, ... < TCON * K - the bound is the
// element count: TCON * K is no multiple of 64 for K = 1 at 160), so every store instruction of the wave covers consecutive dwords.  The touch
// part keeps each lane's contacts in registers, tests their geoms against the pair's bitmasks (kernel arguments), accumulates the lane's own
// contacts first and reduces once per quantity with the primitives of wave.hpp.  No atomics, no LDS round trip, no LDS beyond TreeLDS.
#undef TREE_CON_PASSES
#define TREE_CON_PASSES ((TCON + WAVE - 1) / WAVE)

namespace TREE_NS {

struct TreeTouchPairs {            // so101_tree_geom_pair, npair of them: bit (g & 31) of word g >> 5
  int npair;
  unsigned int a[TOUCH_MAX_PAIRS][8], b[TOUCH_MAX_PAIRS][8];
};

DEV bool tree_touch_member(const unsigned int* mask, int g) { return g >= 0 && ((mask[(g >> 5) & 7] >> (g & 31)) & 1u) != 0u; }

// K floats per contact of entry i from word `src` of TCon; slots >= ncon get `fill`
template <int K>
DEV void tree_store_contact_field(float* out, size_t i, const TreeLDS& L, int src, int ncon, float fill) {
  if (!out) return;
  float* o = out + i * (size_t)(TCON * K);
  for (int idx = wave_lane(); idx < TCON * K; idx += WAVE) {
    int k = idx / K, c = idx - k * K;
    o[idx] = k < ncon ? ((const float*)&L.con[k])[src + c] : fill;
  }
}

template <int K>
DEV void tree_fill_contact_field(float* out, size_t i, float fill) {
  if (!out) return;
  float* o = out + i * (size_t)(TCON * K);
  for (int idx = wave_lane(); idx < TCON * K; idx += WAVE) o[idx] = fill;
}

// an entry whose env index lies outside the batch reads nothing (the convention of so101_contacts): count -1, flags 0, geoms -1, the touch
// part's counts 0, every float NaN
DEV void tree_contacts_outside(size_t i, int npair, const ContactOut& O) {
  int lane = wave_lane();
  const float nan = __builtin_nanf("");
  if (lane == 0) { if (O.count) O.count[i] = -1; if (O.flags) O.flags[i] = 0; }
  if (O.geom) for (int idx = lane; idx < TCON * 2; idx += WAVE) O.geom[i * (size_t)(TCON * 2) + idx] = -1;
  tree_fill_contact_field<1>(O.dist, i, nan);
  tree_fill_contact_field<3>(O.pos, i, nan);
  tree_fill_contact_field<9>(O.frame, i, nan);
  tree_fill_contact_field<6>(O.force, i, nan);
  if (lane < npair) {
    size_t p = i * (size_t)npair + lane;
    if (O.pair_count) O.pair_count[p] = 0;
    if (O.pair_dist) O.pair_dist[p] = nan;
    if (O.pair_normal) O.pair_normal[p] = nan;
    if (O.pair_force) { O.pair_force[3 * p] = nan; O.pair_force[3 * p + 1] = nan; O.pair_force[3 * p + 2] = nan; }
  }
}

// entries i0 .. i0 + gridDim.x - 1 of the call; with forces at most N of them per launch (the scratch slices)
__global__ void __launch_bounds__(64) k_tree_contacts(const TreeModel* tm, const DevModel* gm, TreeBuffers B, int N, int iterations, float tolerance, const int* env_index, int i0,
                                                      int forces, TreeTouchPairs T, ContactOut O) {
  BLOCK_SHARED(TreeLDS, L);
  const size_t i = (size_t)i0 + blockIdx.x;
  const int lane = wave_lane();
  const int e = env_index ? wave_uniform_i(env_index[i]) : (int)i;
  if (e < 0 || e >= N) { tree_contacts_outside(i, T.npair, O); return; }
  if (lane == 0) L.flags = 0;
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
  if (lane == 0) { if (O.count) O.count[i] = ncon; if (O.flags) O.flags[i] = L.flags; }
  // ---- per-contact arrays
  if (O.geom) {
    for (int idx = lane; idx < TCON * 2; idx += WAVE) {
      int k = idx >> 1;
      O.geom[i * (size_t)(TCON * 2) + idx] = k < ncon ? ((idx & 1) ? L.con[k].g2 : L.con[k].g1) : -1;
    }
  }
  tree_store_contact_field<1>(O.dist, i, L, (int)(offsetof(TCon, dist) / 4), ncon, __builtin_inff());
  tree_store_contact_field<3>(O.pos, i, L, (int)(offsetof(TCon, pos) / 4), ncon, 0.f);
  tree_store_contact_field<9>(O.frame, i, L, (int)(offsetof(TCon, frame) / 4), ncon, 0.f);
  const bool solved = forces && nrow > 0;
  if (forces && O.force) {
    float* o = O.force + i * (size_t)(TCON * 6);
    for (int idx = lane; idx < TCON * 6; idx += WAVE) {
      int k = idx / 6, j = idx - k * 6;
      float v = 0.f;
      if (solved && k < nkeep && j < L.con[k].dim) v = G.ef[L.con[k].row + j];
      o[idx] = v;
    }
  }
  // ---- touch: lane = contact (TREE_CON_PASSES of them per lane), one wave reduction per quantity and pair
  const int npair = T.npair;
  if (npair == 0) return;
  int g1[TREE_CON_PASSES], g2[TREE_CON_PASSES];
  float dist[TREE_CON_PASSES], fn[TREE_CON_PASSES], fw[TREE_CON_PASSES][3];
#pragma unroll
  for (int q = 0; q < TREE_CON_PASSES; q++) {
    const int k = q * WAVE + lane;
    g1[q] = -1; g2[q] = -1; dist[q] = __builtin_inff(); fn[q] = 0.f; fw[q][0] = fw[q][1] = fw[q][2] = 0.f;
    if (k < ncon) {
      const TCon& c = L.con[k];
      g1[q] = c.g1; g2[q] = c.g2; dist[q] = c.dist;
      if (solved && k < nkeep) {
        float f[3];
#pragma unroll
        for (int j = 0; j < 3; j++) f[j] = j < c.dim ? G.ef[c.row + j] : 0.f;
        fn[q] = f[0];
#pragma unroll
        for (int j = 0; j < 3; j++) fw[q][j] = c.frame[j] * f[0] + c.frame[3 + j] * f[1] + c.frame[6 + j] * f[2];      // R^T f[0:3]: the force on geom2's body, world frame
      }
    }
  }
  for (int p = 0; p < npair; p++) {
    int cnt = 0;
    float dmin = __builtin_inff(), sn = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
    for (int q = 0; q < TREE_CON_PASSES; q++) {
      // first order that holds: group A has geom1 (the force on A is -R^T f), otherwise group A has geom2 (+R^T f); a slot beyond count has geoms -1
      const bool ab = tree_touch_member(T.a[p], g1[q]) && tree_touch_member(T.b[p], g2[q]);
      const bool ba = !ab && tree_touch_member(T.a[p], g2[q]) && tree_touch_member(T.b[p], g1[q]);
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
}  // namespace TREE_NS
