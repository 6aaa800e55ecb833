// Proximity sensing (so101_proximity and so101_tree_proximity of include/so101.h): the smallest signed distance between two groups of geoms, with
// the closest points, for thousands of (entry, group pair) per call.  One wavefront per (entry, pair): block b serves entry b / npair and pair
// b % npair.  The pass is the engine's load_state, the joint values from `q` when given, kinematics - no dynamics, no constraint code, and nothing
// is stored to a bound buffer.
//
// Candidates.  The model's admitted pair list (pair_packed, what broadphase() walks) is read PROX_ROUND pairs at a time, lane = pair.  A pair
// is a member when one geom is in group a and the other in b; the order "geom1 in a" is tried first.  Each member gets a LOWER bound of its
// signed distance from the bounding spheres (centre distance minus both radii; for the plane the centre's height minus the radius), less
// PROX_BOUND_SLACK for the rounding of the bound itself.  Members whose bound is below max_dist go to a list in LDS, in pair order.  The wave
// then takes the smallest bound left, stops when it is above the best distance so far, otherwise runs the exact query with all 64 lanes.
// Ties go to the earlier pair: a later pair replaces the best only when strictly smaller.  The spheres also bound a penetration from below:
// moving one geom until the spheres part separates the geoms, so the minimum translation is at most the spheres' overlap.
//
// Exact query of a separated pair: GJK on the Minkowski difference A - B with support() / mdsupport() of so101_geom.hpp (hull scans across the
// 64 lanes, from global memory: NoCache, hulls of any size).  Spheres and capsules enter as their CORE (a point, a segment: the same geom with
// radius 0) and the radii are subtracted afterwards, so the cores are polytopes, the iteration is finite and the answer exact.  A plane is closed
// form: the other geom's support along the negated normal.  The simplex holds at most four points with their witnesses; every index into it is
// a compile-time constant (selects, no scratch memory).
//
// Termination.  With v the closest point of the simplex to the origin and w the new support point, v.w / |v| is a lower bound of the distance,
// so |v|^2 - v.w <= PROX_GJK_EPS |v|^2 bounds the error by PROX_GJK_EPS |v|: 1e-6 of at most a few metres, below fp32's own resolution of the
// points (6e-8 relative of ~1 m coordinates).  Polytopes end earlier, when the support point is one the simplex already has.  fp32 can also stall
// with |v| not decreasing; that ends the iteration as converged (the points' resolution is reached).  PROX_GJK_MAXIT = 48 is the cap: a polytope
// pair ends after at most a few more iterations than its closest features have vertices, and no (entry, pair) of the tests or of 4096 envs of the
// headline workload reached it; reaching it sets flags bit 2 and the value is an upper bound.
//
// Penetration.  When the simplex encloses the origin, or the distance is below PROX_HANDOVER = 1e-4 m, the pair goes to narrow_pair() - the step's
// own narrowphase - and its deepest contact is reported (flags bit 1): dist < 0, the contact normal, both points the contact position offset by
// -+ dist / 2 along it.  Below 1e-4 m the fp32 simplex cannot tell a resting contact (penetration 1e-4 .. 1e-3 m here) from a gap reliably, and
// "proximity < 0" must be what "touch" says.  Where narrow_pair() finds no contact the GJK result stands (an enclosed origin: distance 0).
//
// This file is the part both engines share: the constants, the GJK, the step of one pair on two loaded geoms (the narrowphase policy a template
// parameter: where a geom's pose comes from and which hull cache the engine's own narrowphase uses are the engine's business), the bound of one
// model pair from the bounding-sphere rows and the output record.  The kernels: k_proximity (so101_proximity.hpp, the SO100 engine) and
// k_tree_proximity (so101_tree_kernels.hpp, the general-tree engine, both builds).
#pragma once
#include "so101_geom.hpp"

#define PROX_ROUND 1024              // model pairs per candidate round (16 per lane); the list lives in the contact slots of the engine's LDS struct
#define PROX_GJK_MAXIT 48
#define PROX_GJK_EPS 1e-6f
#define PROX_HANDOVER 1e-4f
#define PROX_BOUND_SLACK 2e-6f
#define PROX_FLAG_PENETRATING 1
#define PROX_FLAG_ITERATIONS 2
#define PROX_FLAG_BEYOND 4
#define PROX_FLAG_OUTSIDE 8

struct ProxResult { float dist, pa[3], pb[3], n[3]; int flags; };      // geom1's point, geom2's point, unit normal geom1 -> geom2

// closest point of the simplex P[0 .. n - 1] (the newest point last) to the origin: weights bw[4] (zero for the points that drop out), `inside`
// when a tetrahedron holds the origin
DEV void prox_simplex(const float (*P)[3], int n, float* bw, bool& inside) {
  inside = false;
  bw[0] = 1.f; bw[1] = 0.f; bw[2] = 0.f; bw[3] = 0.f;
  if (n == 2) {
    float wt[3], t; seg_origin(P[0], P[1], wt, &t);
    bw[0] = 1.f - t; bw[1] = t;
  } else if (n == 3) {
    float wt[3], b3[3]; origin_tri_dist2(P[0], P[1], P[2], wt, b3);
    bw[0] = b3[0]; bw[1] = b3[1]; bw[2] = b3[2];
  } else if (n == 4) {
    // origin and the fourth vertex on the same side of every face: inside.  A flat tetrahedron (|sd| tiny) is never "inside".
    bool in = true;
#pragma unroll
    for (int f = 0; f < 4; f++) {
      const float* a = P[(f + 1) & 3]; const float* b = P[(f + 2) & 3]; const float* c = P[(f + 3) & 3]; const float* d = P[f];
      float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]}, nn[3];
      cross3(nn, e1, e2);
      float sd = nn[0] * (d[0] - a[0]) + nn[1] * (d[1] - a[1]) + nn[2] * (d[2] - a[2]), so = -dot3(nn, a);
      float scale = sqrtf(dot3(nn, nn)) * 1e-7f;
      in = in && (fabsf(sd) > scale) && (sd * so > 0.f);
    }
    inside = in;
    // the three faces that hold the newest point (the fourth is the previous simplex, whose closest point is the previous v)
    float wt[3], b3[3], best;
    best = origin_tri_dist2(P[0], P[1], P[3], wt, b3);
    bw[0] = b3[0]; bw[1] = b3[1]; bw[2] = 0.f; bw[3] = b3[2];
    float e = origin_tri_dist2(P[0], P[2], P[3], wt, b3);
    if (e < best) { best = e; bw[0] = b3[0]; bw[1] = 0.f; bw[2] = b3[1]; bw[3] = b3[2]; }
    e = origin_tri_dist2(P[1], P[2], P[3], wt, b3);
    if (e < best) { best = e; bw[0] = 0.f; bw[1] = b3[0]; bw[2] = b3[1]; bw[3] = b3[2]; }
  }
}

// GJK distance of the cores of G1 and G2 (rs = the radii taken off: the result is the surface distance).  `cutoff`: the query is given up
// (returns false) as soon as its own lower bound exceeds it - the pair cannot win.  Otherwise R holds the distance (>= 0 when separated; flag
// bit 1 and nothing else valid when the cores touch or the surfaces are within PROX_HANDOVER: the caller asks narrow_pair) and the witnesses.
DEV bool prox_gjk(const DevModel* m, const GeomW& G1, const GeomW& G2, float r1, float r2, float cutoff, ProxResult& R) {
  const NoCache H{};
  const float org[3] = {0.f, 0.f, 0.f}, rs = r1 + r2;
  float sv[4][3], sa[4][3], sb[4][3], bw[4] = {1.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) { sv[i][k] = 0.f; sa[i][k] = 0.f; sb[i][k] = 0.f; }
  float v[3] = {G1.c[0] - G2.c[0], G1.c[1] - G2.c[1], G1.c[2] - G2.c[2]};
  if (!(dot3(v, v) > 1e-20f)) { v[0] = 1.f; v[1] = 0.f; v[2] = 0.f; }
  int n = 0;
  bool overlap = false, capped = true;
#pragma unroll 1
  for (int it = 0; it < PROX_GJK_MAXIT; it++) {
    MV w;
    const float dir[3] = {-v[0], -v[1], -v[2]};
    mdsupport<NoCache>(m, G1, G2, dir, org, w, H, H);
    const float vv = dot3(v, v), vw = dot3(v, w.v);
    if (n > 0) {
      // (v.w / |v| - rs > cutoff, without the division and only where v.w > 0)
      const float lim = (cutoff + rs) * sqrtf(vv);
      if (vw > 0.f && cutoff + rs > 0.f && vw > lim * (1.f + 1e-5f) + 1e-12f) return false;
      bool dup = false;
#pragma unroll
      for (int i = 0; i < 4; i++) dup = dup || (i < n && sv[i][0] == w.v[0] && sv[i][1] == w.v[1] && sv[i][2] == w.v[2]);
      if (dup || vv - vw <= PROX_GJK_EPS * vv) { capped = false; break; }
    }
    // the new point goes last (n < 4 here: a full simplex either held the origin or dropped a point)
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (i == n) {
#pragma unroll
        for (int k = 0; k < 3; k++) { sv[i][k] = w.v[k]; sa[i][k] = w.a[k]; sb[i][k] = w.b[k]; }
      }
    n++;
    bool inside;
    prox_simplex(sv, n, bw, inside);
    if (inside) { overlap = true; capped = false; break; }
    // keep the points with a positive weight, in their order; v = their combination
    float nv[4][3], na[4][3], nb[4][3], nw[4];
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) { nw[i] = 0.f;
#pragma unroll
      for (int k = 0; k < 3; k++) { nv[i][k] = 0.f; na[i][k] = 0.f; nb[i][k] = 0.f; } }
#pragma unroll
    for (int s = 0; s < 4; s++) {
      const bool keep = s < n && bw[s] > 0.f;
#pragma unroll
      for (int d = 0; d < 4; d++)
        if (keep && d == cnt) {
          nw[d] = bw[s];
#pragma unroll
          for (int k = 0; k < 3; k++) { nv[d][k] = sv[s][k]; na[d][k] = sa[s][k]; nb[d][k] = sb[s][k]; }
        }
      cnt += keep ? 1 : 0;
    }
    if (cnt == 0) { overlap = true; capped = false; break; }          // (non-finite weights: nothing to go on with)
    const float wsum = nw[0] + nw[1] + nw[2] + nw[3], inv = 1.f / wsum;
    float x[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; i++) { bw[i] = nw[i] * inv;
#pragma unroll
      for (int k = 0; k < 3; k++) { sv[i][k] = nv[i][k]; sa[i][k] = na[i][k]; sb[i][k] = nb[i][k]; x[k] += bw[i] * nv[i][k]; } }
    n = cnt;
    // v is orthogonal to the sub-simplex that holds it.  The weighted sum has the rounding of the points (6e-8 of ~1 m coordinates), which is
    // a direction error of 1e-4 rad at a distance of a millimetre; the simplex's own edges (centimetres and more) give the direction to 1e-6:
    // a triangle's normal scaled to the plane's distance, a segment's foot point made orthogonal to it.  (Sliver triangles keep the sum.)
    if (cnt == 3) {
      const float e1[3] = {nv[1][0] - nv[0][0], nv[1][1] - nv[0][1], nv[1][2] - nv[0][2]}, e2[3] = {nv[2][0] - nv[0][0], nv[2][1] - nv[0][1], nv[2][2] - nv[0][2]};
      float nn[3]; cross3(nn, e1, e2);
      const float q = dot3(nn, nn);
      if (q > 1e-4f * dot3(e1, e1) * dot3(e2, e2) && q > 1e-30f) {
        const float s = (nn[0] * (bw[0] * nv[0][0] + bw[1] * nv[1][0] + bw[2] * nv[2][0]) + nn[1] * (bw[0] * nv[0][1] + bw[1] * nv[1][1] + bw[2] * nv[2][1]) +
                         nn[2] * (bw[0] * nv[0][2] + bw[1] * nv[1][2] + bw[2] * nv[2][2])) / q;
        x[0] = s * nn[0]; x[1] = s * nn[1]; x[2] = s * nn[2];
      }
    } else if (cnt == 2) {
      const float e[3] = {nv[1][0] - nv[0][0], nv[1][1] - nv[0][1], nv[1][2] - nv[0][2]};
      const float q = dot3(e, e);
      if (q > 1e-30f) { const float s = dot3(x, e) / q; x[0] -= s * e[0]; x[1] -= s * e[1]; x[2] -= s * e[2]; }
    }
    const float xx = dot3(x, x);
    v[0] = x[0]; v[1] = x[1]; v[2] = x[2];
    if (!(xx > 1e-16f)) { overlap = true; capped = false; break; }   // the cores touch (1e-8 m)
    if (it > 0 && !(xx < vv)) { capped = false; break; }             // no progress left in fp32
    if (n == 4) { overlap = true; capped = false; break; }           // (a full simplex that does not hold the origin: degenerate, let narrow_pair decide)
  }
  float pa[3] = {0.f, 0.f, 0.f}, pb[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) { pa[k] += bw[i] * sa[i][k]; pb[k] += bw[i] * sb[i][k]; }
  // the separation is -v (A towards B); the witnesses are set at that distance about their midpoint, so that pb - pa = dist * n to rounding
  const float len = sqrtf(dot3(v, v));
  const float il = len > 1e-30f ? 1.f / len : 0.f;
  R.flags = capped ? PROX_FLAG_ITERATIONS : 0;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    R.n[k] = -v[k] * il;
    const float mid = 0.5f * (pa[k] + pb[k]);
    R.pa[k] = mid - (0.5f * len - r1) * R.n[k]; R.pb[k] = mid + (0.5f * len - r2) * R.n[k];
  }
  R.dist = len - rs;
  if (overlap || !(R.dist >= PROX_HANDOVER)) {
    R.flags |= PROX_FLAG_PENETRATING;
    if (overlap) { R.dist = 0.f;
#pragma unroll
      for (int k = 0; k < 3; k++) { R.pb[k] = R.pa[k]; } }
    R.dist = fmaxf(R.dist, 0.f);
  }
  return true;
}

// one admitted pair (geom types ordered, as in the pair list) on geoms the engine has loaded: false when the pair is farther than `cutoff`.
// Cache / GP: the policies of the engine's own narrowphase - a near pair reports what that narrowphase reports at the same state.
template <class Cache, class GP>
DEV bool prox_pair_geoms(const DevModel* m, const GeomW& G1, const GeomW& G2, int g1, int g2, float cutoff, ProxResult& R) {
  bool near;
  if (G1.type == G_PLANE) {
    const NoCache H{};
    const float nrm[3] = {G1.R[2], G1.R[5], G1.R[8]}, dn[3] = {-nrm[0], -nrm[1], -nrm[2]};
    float s[3]; support<NoCache>(m, G2, dn, s, H);
    const float d = nrm[0] * (s[0] - G1.p[0]) + nrm[1] * (s[1] - G1.p[1]) + nrm[2] * (s[2] - G1.p[2]);
    R.dist = d; R.flags = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) { R.n[k] = nrm[k]; R.pb[k] = s[k]; R.pa[k] = s[k] - d * nrm[k]; }
    near = !(d >= PROX_HANDOVER);
    if (near) { R.dist = fmaxf(d, 0.f); if (!(d > 0.f)) { R.pa[0] = s[0]; R.pa[1] = s[1]; R.pa[2] = s[2]; } }
  } else {
    GeomW C1 = G1, C2 = G2;
    float r1 = 0.f, r2 = 0.f;
    if (G1.type == G_SPHERE || G1.type == G_CAPSULE) { r1 = G1.size[0]; C1.size[0] = 0.f; }
    if (G2.type == G_SPHERE || G2.type == G_CAPSULE) { r2 = G2.size[0]; C2.size[0] = 0.f; }
    if (!prox_gjk(m, C1, C2, r1, r2, cutoff, R)) return false;
    near = (R.flags & PROX_FLAG_PENETRATING) != 0;
    R.flags &= ~PROX_FLAG_PENETRATING;
  }
  if (near) {
    PairContacts pc;
    narrow_pair<Cache, GP>(m, G1, G2, g1, g2, pc);
    float dmin = 0.f; bool any = false;
    float pos[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NCPP; j++) {
      const bool take = ((pc.valid >> j) & 1u) && (!any || pc.dist[j] < dmin);
      if (take) { dmin = pc.dist[j]; pos[0] = pc.pos[j][0]; pos[1] = pc.pos[j][1]; pos[2] = pc.pos[j][2]; any = true; }
    }
    if (any) {
      R.dist = dmin; R.flags = PROX_FLAG_PENETRATING;
#pragma unroll
      for (int k = 0; k < 3; k++) { R.n[k] = pc.nrm[k]; R.pa[k] = pos[k] - 0.5f * dmin * pc.nrm[k]; R.pb[k] = pos[k] + 0.5f * dmin * pc.nrm[k]; }
    }
  }
  return true;
}

// Lower bound of the signed distance of model pair `w` (geoms g1, g2) from the bounding-sphere rows an engine keeps in the geom-box slots of its LDS
// struct: rows 0-2 the centre, row 3 the radius; a plane keeps its point in rows 0-2 and its normal in rows 3-5 (bit 16 of the pair word says
// that geom1 is a plane).  PROX_BOUND_SLACK covers the rounding of the bound itself.
template <class LDS>
DEV float prox_bound(const LDS& L, unsigned int w, int g1, int g2) {
  const float c1[3] = {L.aabb[0][g1], L.aabb[1][g1], L.aabb[2][g1]}, c2[3] = {L.aabb[0][g2], L.aabb[1][g2], L.aabb[2][g2]};
  const float d[3] = {c2[0] - c1[0], c2[1] - c1[1], c2[2] - c1[2]};
  float lb;
  if ((w >> 16) & 1u) lb = L.aabb[3][g1] * d[0] + L.aabb[4][g1] * d[1] + L.aabb[5][g1] * d[2] - L.aabb[3][g2];
  else lb = sqrtf(dot3(d, d)) - L.aabb[3][g1] - L.aabb[3][g2];
  return lb - PROX_BOUND_SLACK * (1.f + fabsf(lb));
}

DEV void prox_store(size_t o, float max_dist, bool found, int ga, int gb, const float* pa, const float* pb, const float* nrm, float dist, int flags, int queries,
                    const ProxOut& O) {
  const int lane = wave_lane();
  if (!found) flags |= PROX_FLAG_BEYOND;
  if (lane == 0) {
    if (O.dist) O.dist[o] = found ? dist : max_dist;
    if (O.flags) O.flags[o] = flags;
    if (O.queries) O.queries[o] = queries;
  }
  // (one lane per word, the values selected by branches: a select chain over the lane index becomes an indexed array in scratch memory)
  if (O.geom) { if (lane == 0) O.geom[2 * o] = found ? ga : -1; if (lane == 1) O.geom[2 * o + 1] = found ? gb : -1; }
  if (O.normal) {
    if (lane == 2) O.normal[3 * o] = found ? nrm[0] : 0.f;
    if (lane == 3) O.normal[3 * o + 1] = found ? nrm[1] : 0.f;
    if (lane == 4) O.normal[3 * o + 2] = found ? nrm[2] : 0.f;
  }
  if (O.point) {
    if (lane == 8) O.point[6 * o] = found ? pa[0] : 0.f;
    if (lane == 9) O.point[6 * o + 1] = found ? pa[1] : 0.f;
    if (lane == 10) O.point[6 * o + 2] = found ? pa[2] : 0.f;
    if (lane == 11) O.point[6 * o + 3] = found ? pb[0] : 0.f;
    if (lane == 12) O.point[6 * o + 4] = found ? pb[1] : 0.f;
    if (lane == 13) O.point[6 * o + 5] = found ? pb[2] : 0.f;
  }
}

// q as joint columns (the general-tree engine): entry i is evaluated with qpos[adr[k]] = q[i][k], k < ncol; the addresses travel in the kernel arguments
#define PROX_MAXCOL 16
struct ProxCols { int ncol; int adr[PROX_MAXCOL]; };
