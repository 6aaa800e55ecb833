// Collision geometry shared by the SO100 engine (so101_device.hpp) and the general-tree engine (so101_tree.hpp): geoms in the world,
// hull caches, support functions, MPR / EPA, the support-bound tables, flat-face scan, patches, narrow_pair.  Both engines and the
// device probes of the test suite (tests/devprims) depend on this file bit for bit: a change here changes every workload's contacts.
// A geom's pose is an argument (load_geom_at); where an engine keeps its poses is its own business.
#pragma once
#include "so101_model.hpp"
#include "wave.hpp"
#include "so101_math.hpp"

// ------------------------------------------------------------------ geometry
// Lane-group policies of the narrowphase.  The query of one geom pair is "uniform" code (every lane of the group
// computes the same portal) around a lane-parallel hull scan.  G64: the whole wavefront works on one pair (fused
// kernels: the env's wave walks its candidates).  G16: one pair per DPP row of 16 lanes, four pairs per wavefront
// (k_narrow): the uniform part is issued once for four pairs, the hull scan takes four times as many steps per pair;
// rows diverge freely (each row's reductions are row-local DPP butterflies, loads become vector loads with a
// row-uniform address).  Both pick the same support vertex (max dot, smallest index), hence bit-identical contacts.
struct G64 {
  static constexpr int N = 64;
  DEV static int sub() { return wave_lane(); }
  DEV static void argmax3(float& val, int& idx, float& x, float& y, float& z) { wave_argmax3(val, idx, x, y, z); }
  DEV static void argmax(float& val, int& idx) { wave_argmax(val, idx); }
  DEV static void argmax_lean(float& val, int& idx) { wave_argmax(val, idx); }
  template <class T> DEV static T ld(const T* p) { return ldc(p); }
  DEV static int uni(int v) { return wave_uniform_i(v); }
};
struct G16 {
  static constexpr int N = 16;
  DEV static int sub() { return wave_lane() & 15; }
  DEV static void argmax3(float& val, int& idx, float& x, float& y, float& z) { row_argmax3(val, idx, x, y, z); }
  DEV static void argmax(float& val, int& idx) { float x = 0.f, y = 0.f, z = 0.f; row_argmax3(val, idx, x, y, z); }
  // the payload-free row reduction (wave.hpp row_argmax): same winner.  The list-backed subsets (HullSub) use it for the five patch reductions of
  // support_multi(); the staged-hull row pass of k_narrow<true> keeps argmax() and with it the code it was measured with.
#if defined(SO101_EMU) && !defined(SO101_EMU_ROW_ARGMAX)      // (a lane-thread emulation header that has the payload form only)
  DEV static void argmax_lean(float& val, int& idx) { argmax(val, idx); }
#else
  DEV static void argmax_lean(float& val, int& idx) { row_argmax(val, idx); }
#endif
  template <class T> DEV static T ld(const T* p) { return *p; }
  DEV static int uni(int v) { return v; }
};

struct GeomW { int type, vadr, vnum; float size[3], R[9], p[3], c[3]; };

// xp/xm: world position and orientation of the geom's dynamic body (ignored for static geoms)
template <class GP = G64>
DEV void load_geom_at(const DevModel* m, int g, const float* xp, const float* xm, GeomW& G) {
  g = GP::uni(g);
  G.type = GP::ld(ldc(&m->geom_type) + g); G.vadr = GP::ld(ldc(&m->geom_vertadr) + g); G.vnum = GP::ld(ldc(&m->geom_vertnum) + g);
  const float* gp = ldc(&m->geom_pos) + 3 * g; const float* gm = ldc(&m->geom_mat) + 9 * g;
  const float* gc = ldc(&m->geom_center) + 3 * g; const float* gs = ldc(&m->geom_size) + 3 * g;
#pragma unroll
  for (int i = 0; i < 3; i++) G.size[i] = GP::ld(gs + i);
  int d = GP::ld(ldc(&m->geom_dyn) + g);
  float lp[3] = {GP::ld(gp), GP::ld(gp + 1), GP::ld(gp + 2)}, lm[9], lc[3] = {GP::ld(gc), GP::ld(gc + 1), GP::ld(gc + 2)};
#pragma unroll
  for (int i = 0; i < 9; i++) lm[i] = GP::ld(gm + i);
  // static geoms go through the same arithmetic with an identity pose (exact: 1*a + 0*b + 0*c == a), so that the
  // geom stays in registers instead of becoming a stack object selected by the branch
  float X[9], P0[3];
#pragma unroll
  for (int i = 0; i < 9; i++) X[i] = d < 0 ? (i % 4 == 0 ? 1.f : 0.f) : xm[i];
#pragma unroll
  for (int i = 0; i < 3; i++) P0[i] = d < 0 ? 0.f : xp[i];
  float t[3]; matvec3(t, X, lp);
#pragma unroll
  for (int i = 0; i < 3; i++) G.p[i] = P0[i] + t[i];
  matmul3(G.R, X, lm);
  float cw[3]; matvec3(cw, G.R, lc);
#pragma unroll
  for (int i = 0; i < 3; i++) G.c[i] = G.p[i] + cw[i];
}

// Hull vertices of one geom held in registers for the duration of a narrowphase query: lane l keeps vertices
// l, l+64, ... (HULL_K of them; 64 * 8 = 512 covers all but four hulls of the SO100 scenes, the rest of those is scanned in memory).  An MPR
// query evaluates ~20-30 support points per geom; reading the hull once instead of once per support call removes
// the vertex traffic (205 -> ~10 vector loads per candidate pair).  Only k_narrow can afford the registers; the fused
// kernels use NoCache and scan memory.  Both variants visit the vertices in the same order with the same
// arithmetic, so they return the same vertex.
#ifndef HULL_K
#define HULL_K 8
#endif
struct HullCache { float x[HULL_K], y[HULL_K], z[HULL_K]; };
struct NoCache {};

template <class GP = G64>
DEV void hull_load(const DevModel* m, const GeomW& G, HullCache& H) {
  // every slot is written (slots beyond the hull, and the caches of primitives, hold zeros): the caches are moved
  // around with selects later, and a select over a never-written register is undefined behaviour for the compiler
#pragma unroll
  for (int j = 0; j < HULL_K; j++) { H.x[j] = 0.f; H.y[j] = 0.f; H.z[j] = 0.f; }
  if (G.type != G_MESH) return;
  int lane = GP::sub();
  const float* x = ldc(&m->vx) + G.vadr; const float* y = ldc(&m->vy) + G.vadr; const float* z = ldc(&m->vz) + G.vadr;
#pragma unroll
  for (int j = 0; j < HULL_K; j++) {
    if (GP::N * j >= G.vnum) break;
    int i = lane + GP::N * j;
    bool v = i < G.vnum;
    H.x[j] = v ? x[i] : 0.f; H.y[j] = v ? y[i] : 0.f; H.z[j] = v ? z[i] : 0.f;
  }
}
template <class GP = G64>
DEV void hull_load(const DevModel*, const GeomW&, NoCache&) {}

// The same cache in LDS (k_narrow, one wavefront per workgroup: round 5).  The register cache above costs 48 VGPRs for the two geoms of a
// pair across the whole query - with the EPA polytope inlined k_narrow needed 256 + 43 spilled - while the kernel used 256 B of its 20 KB LDS
// share.  Here the first HULL_LDS_MAX vertices of a hull are staged by the kernel (so101_narrow.hpp: all hulls of a work-item chunk at once,
// behind ONE memory round trip) as x[n] | y[n] | z[n] with n = 256 or 512 slots, and a support scan reads them four vertices per lane and
// instruction (ds_read_b128: lane l takes vertices 256 J + 4 l + 0..3, in increasing index order, so "largest dot product, smallest index"
// picks the vertex every other variant picks).
#define HULL_LDS_MAX 512
struct HullLDS { float* p; int n; };      // p: [3][n] floats in LDS (16-byte aligned), n: slots per coordinate (0: nothing staged)
DEV int hull_lds_slots(int type, int vnum) { return type != G_MESH ? 0 : (vnum <= 256 ? 256 : HULL_LDS_MAX); }
// the loads of one hull (issued, not waited for) and their LDS stores: split so that a caller can issue the loads of several hulls first
template <int NJ> struct HullStage { float x[NJ], y[NJ], z[NJ]; };
template <int NJ>
DEV void hull_stage_issue(const DevModel* m, int vadr, int vnum, int j0, HullStage<NJ>& T) {
  int lane = wave_lane();
  const float* x = ldc(&m->vx) + vadr; const float* y = ldc(&m->vy) + vadr; const float* z = ldc(&m->vz) + vadr;
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    int i = lane + WAVE * (j0 + j);
    bool v = i < vnum;
    T.x[j] = v ? x[i] : 0.f; T.y[j] = v ? y[i] : 0.f; T.z[j] = v ? z[i] : 0.f;
  }
}
template <int NJ>
DEV void hull_stage_store(const HullLDS& H, int vnum, int j0, const HullStage<NJ>& T) {
  int lane = wave_lane();
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    int i = lane + WAVE * (j0 + j);
    if (WAVE * (j0 + j) < H.n) { H.p[i] = T.x[j]; H.p[H.n + i] = T.y[j]; H.p[2 * H.n + i] = T.z[j]; }
  }
}
// one hull into its LDS slots (loads of a 256-slot block in flight together)
DEV void hull_stage(const DevModel* m, int vadr, int vnum, const HullLDS& H) {
  for (int j0 = 0; WAVE * j0 < H.n; j0 += 4) {
    HullStage<4> T;
    hull_stage_issue<4>(m, vadr, vnum, j0, T);
    hull_stage_store<4>(H, vnum, j0, T);
  }
}
template <class GP = G64>
DEV void hull_load(const DevModel* m, const GeomW& G, HullLDS& H) { if (H.n) hull_stage(m, G.vadr, G.vnum, H); }
// uniform values parked in LDS across a phase that does not need them (k_narrow: the candidate face across the iterative query, the portal
// across the EPA expansion): the register allocator otherwise keeps them in VGPRs, 64 copies of each, or spills them to scratch memory
#define NARROW_PARK_WORDS 192
DEV float* narrow_park_store() { __shared__ __attribute__((aligned(16))) float park[NARROW_PARK_WORDS]; return park; }

DEV void select_geom(bool first, const GeomW& A, const GeomW& B, GeomW& o) {
  o.type = first ? A.type : B.type; o.vadr = first ? A.vadr : B.vadr; o.vnum = first ? A.vnum : B.vnum;
#pragma unroll
  for (int i = 0; i < 3; i++) { o.size[i] = first ? A.size[i] : B.size[i]; o.p[i] = first ? A.p[i] : B.p[i]; o.c[i] = first ? A.c[i] : B.c[i]; }
#pragma unroll
  for (int i = 0; i < 9; i++) o.R[i] = first ? A.R[i] : B.R[i];
}
DEV void select_hull(bool first, const HullCache& A, const HullCache& B, HullCache& o) {
#pragma unroll
  for (int j = 0; j < HULL_K; j++) { o.x[j] = first ? A.x[j] : B.x[j]; o.y[j] = first ? A.y[j] : B.y[j]; o.z[j] = first ? A.z[j] : B.z[j]; }
}
DEV void select_hull(bool, const NoCache&, const NoCache&, NoCache&) {}
DEV void select_hull(bool first, const HullLDS& A, const HullLDS& B, HullLDS& o) { o.p = first ? A.p : B.p; o.n = first ? A.n : B.n; }
// A SUBSET of a hull in registers (round 6, k_narrow's fast path for a flat face against a hull): the entries of one cell of the hull's
// support-vertex lists (DevModel::hl_entry), two per lane at most, in increasing index order (entry l, then entry l + 64); slots beyond the
// list carry the index 0x7fffffff.  Valid for the directions of that cell (widened by 4e-3 rad) only: there the largest dot product over the
// subset is the largest over the hull, attained by the same vertices - support() and support_multi() return the same point bit for bit.
struct HullSub { float x[2], y[2], z[2]; int i[2]; };
template <class C> struct is_hull_sub { static constexpr bool value = false; };
template <> struct is_hull_sub<HullSub> { static constexpr bool value = true; };
DEV void select_hull(bool first, const HullSub& A, const HullSub& B, HullSub& o) {
#pragma unroll
  for (int j = 0; j < 2; j++) { o.x[j] = first ? A.x[j] : B.x[j]; o.y[j] = first ? A.y[j] : B.y[j]; o.z[j] = first ? A.z[j] : B.z[j]; o.i[j] = first ? A.i[j] : B.i[j]; }
}
// The subset of ONE ROW of 16 lanes (policy G16, k_narrow's list row pass): entries sub and sub + 16 of a list of at most HL_ROW_MAX, sub = lane & 15 - in
// increasing index order per lane like the whole-wave subset; E = the list's first entry (x, y, z, index as bits), cnt = its length (0: every slot empty).
// The loads are issued together and nothing here waits for them.
#define HL_ROW_MAX 32
DEV void hull_sub_row_load(const float* E, int cnt, HullSub& S) {
  const int sub = wave_lane() & 15;
#pragma unroll
  for (int q = 0; q < 2; q++) {
    int k = sub + 16 * q;
    bool in = k < cnt;
    float4 ev; ev.x = 0.f; ev.y = 0.f; ev.z = 0.f; ev.w = 0.f;
    if (in) ev = *(const float4*)(E + 4 * (size_t)k);
    S.x[q] = ev.x; S.y[q] = ev.y; S.z[q] = ev.z; S.i[q] = in ? __float_as_int(ev.w) : 0x7fffffff;
  }
}
// cell of the cube map a direction (any length, geom frame) falls into: face 2 a + (negative), then HL_GRID x HL_GRID along the axes a + 1, a + 2
DEV int hl_cell(const float* dl) {
  float a0 = fabsf(dl[0]), a1 = fabsf(dl[1]), a2 = fabsf(dl[2]);
  int ax = a0 >= a1 ? (a0 >= a2 ? 0 : 2) : (a1 >= a2 ? 1 : 2);
  float dm = ax == 0 ? dl[0] : (ax == 1 ? dl[1] : dl[2]);
  float du = ax == 0 ? dl[1] : (ax == 1 ? dl[2] : dl[0]);
  float dv = ax == 0 ? dl[2] : (ax == 1 ? dl[0] : dl[1]);
  float inv = 1.f / fmaxf(fabsf(dm), 1e-20f);
  float gu = fminf(fmaxf((du * inv + 1.f) * (0.5f * HL_GRID), 0.f), (float)HL_GRID), gv = fminf(fmaxf((dv * inv + 1.f) * (0.5f * HL_GRID), 0.f), (float)HL_GRID);
  int iu = (int)gu; iu = iu > HL_GRID - 1 ? HL_GRID - 1 : iu;
  int iv = (int)gv; iv = iv > HL_GRID - 1 ? HL_GRID - 1 : iv;
  return ((2 * ax + (dm < 0.f ? 1 : 0)) * HL_GRID + iu) * HL_GRID + iv;
}
template <class C> struct is_hull_lds { static constexpr bool value = false; };
template <> struct is_hull_lds<HullLDS> { static constexpr bool value = true; };

// support point (world) of G in world direction dir; wave-parallel over hull vertices for meshes
template <class Cache, class GP = G64>
DEV void support(const DevModel* m, const GeomW& G, const float* dir, float* out, const Cache& H) {
  float dl[3]; matTvec3(dl, G.R, dir);
  float loc[3] = {0.f, 0.f, 0.f};
  if (G.type == G_MESH) {
    int lane = GP::sub();
    // each lane scans vertices lane, lane+64, ... (coalesced SoA loads) and keeps its best vertex in registers;
    // the wave-level argmax then broadcasts the winner with v_readlane (no second memory access, and a
    // non-finite direction of a diverged state can never index out of range)
    float best = -3.0e38f, bx = 0.f, by = 0.f, bz = 0.f; int bi = 0x7fffffff;
    const float* x = ldc(&m->vx) + G.vadr; const float* y = ldc(&m->vy) + G.vadr; const float* z = ldc(&m->vz) + G.vadr;
    int first = lane;
    if constexpr (is_hull_sub<Cache>::value) {
#pragma unroll
      for (int k = 0; k < 2; k++) {
        int i = H.i[k];
        float d = H.x[k] * dl[0] + H.y[k] * dl[1] + H.z[k] * dl[2];
        if (i < G.vnum && d > best) { best = d; bi = i; bx = H.x[k]; by = H.y[k]; bz = H.z[k]; }
      }
      first = G.vnum;                                  // (nothing else to scan)
    } else if constexpr (is_hull_lds<Cache>::value) {
      const float4* X4 = (const float4*)H.p; const float4* Y4 = (const float4*)(H.p + H.n); const float4* Z4 = (const float4*)(H.p + 2 * H.n);
      auto block = [&](int J) {
        float4 xv = X4[GP::N * J + lane], yv = Y4[GP::N * J + lane], zv = Z4[GP::N * J + lane];
        float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ys[4] = {yv.x, yv.y, yv.z, yv.w}, zs[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
          int i = 4 * GP::N * J + 4 * lane + k;
          float d = xs[k] * dl[0] + ys[k] * dl[1] + zs[k] * dl[2];
          if (i < G.vnum && d > best) { best = d; bi = i; bx = xs[k]; by = ys[k]; bz = zs[k]; }
        }
      };
      if constexpr (GP::N == WAVE) {
#pragma unroll
        for (int J = 0; J < HULL_LDS_MAX / (4 * WAVE); J++) {
          if (4 * WAVE * J >= G.vnum || 4 * WAVE * J >= H.n) break;
          block(J);
        }
      } else {
        // a row of 16 lanes per pair (k_narrow's row pass): 64 vertices per step, trip count per row
        const int lim = G.vnum < H.n ? G.vnum : H.n;
#pragma unroll 1
        for (int J = 0; 4 * GP::N * J < lim; J++) block(J);
      }
      first = lane + H.n;
    } else if constexpr (sizeof(Cache) >= sizeof(HullCache)) {
#pragma unroll
      for (int j = 0; j < HULL_K; j++) {
        if (GP::N * j >= G.vnum) break;
        int i = lane + GP::N * j;
        float X = H.x[j], Y = H.y[j], Z = H.z[j];
        float d = X * dl[0] + Y * dl[1] + Z * dl[2];
        if (i < G.vnum && d > best) { best = d; bi = i; bx = X; by = Y; bz = Z; }
      }
      first = lane + GP::N * HULL_K;
    }
#pragma unroll 4
    for (int i = first; i < G.vnum; i += GP::N) {
      float X = x[i], Y = y[i], Z = z[i];
      float d = X * dl[0] + Y * dl[1] + Z * dl[2];
      if (d > best) { best = d; bi = i; bx = X; by = Y; bz = Z; }
    }
    GP::argmax3(best, bi, bx, by, bz);
    loc[0] = bx; loc[1] = by; loc[2] = bz;
  } else if (G.type == G_BOX) {
#pragma unroll
    for (int i = 0; i < 3; i++) loc[i] = dl[i] >= 0.f ? G.size[i] : -G.size[i];
  } else if (G.type == G_CAPSULE) {
    float n = sqrtf(dot3(dl, dl));
    if (n > MINVAL_F) { float s = G.size[0] / n; loc[0] = s * dl[0]; loc[1] = s * dl[1]; loc[2] = s * dl[2]; }
    loc[2] += dl[2] >= 0.f ? G.size[1] : -G.size[1];
  } else if (G.type == G_CYLINDER) {
    float n = sqrtf(dl[0] * dl[0] + dl[1] * dl[1]);
    if (n > MINVAL_F) { float s = G.size[0] / n; loc[0] = s * dl[0]; loc[1] = s * dl[1]; }
    loc[2] = dl[2] >= 0.f ? G.size[1] : -G.size[1];
  } else if (G.type == G_SPHERE) {
    float n = sqrtf(dot3(dl, dl));
    if (n > MINVAL_F) { float s = G.size[0] / n; loc[0] = s * dl[0]; loc[1] = s * dl[1]; loc[2] = s * dl[2]; }
  }
  float w[3]; matvec3(w, G.R, loc);
  out[0] = G.p[0] + w[0]; out[1] = G.p[1] + w[1]; out[2] = G.p[2] + w[2];
}

struct MV { float v[3], a[3], b[3]; };

template <class Cache, class GP = G64>
DEV void mdsupport(const DevModel* m, const GeomW& G1, const GeomW& G2, const float* dir, const float* org, MV& o,
                   const Cache& H1, const Cache& H2) {
  float nd[3] = {-dir[0], -dir[1], -dir[2]};
  support<Cache, GP>(m, G1, dir, o.a, H1);
  support<Cache, GP>(m, G2, nd, o.b, H2);
#pragma unroll
  for (int i = 0; i < 3; i++) { o.a[i] -= org[i]; o.b[i] -= org[i]; o.v[i] = o.a[i] - o.b[i]; }
}

DEV bool isz(float x) { return fabsf(x) < EPS_F; }

// origin to segment P0-P1: squared distance, closest point and the parameter t (weight of P1)
DEV float seg_origin(const float* P0, const float* P1, float* wt, float* tout) {
  float dd[3] = {P1[0] - P0[0], P1[1] - P0[1], P1[2] - P0[2]};
  float t = -dot3(P0, dd) / fmaxf(dot3(dd, dd), 1e-30f);
  t = fminf(fmaxf(t, 0.f), 1.f);
  wt[0] = P0[0] + t * dd[0]; wt[1] = P0[1] + t * dd[1]; wt[2] = P0[2] + t * dd[2];
  *tout = t;
  return dot3(wt, wt);
}

// squared distance of the origin to triangle (x0,B,C); wit = closest point, bw = its barycentric weights
DEV float origin_tri_dist2(const float* x0, const float* B, const float* C, float* wit, float* bw) {
  float d1[3] = {B[0] - x0[0], B[1] - x0[1], B[2] - x0[2]}, d2[3] = {C[0] - x0[0], C[1] - x0[1], C[2] - x0[2]};
  float v = dot3(d1, d1), w = dot3(d2, d2), p = dot3(x0, d1), q = dot3(x0, d2), r = dot3(d1, d2);
  float den = w * v - r * r, sp = -1.f, tp = -1.f;
  if (fabsf(den) > 1e-30f) { sp = (q * r - w * p) / den; tp = (-sp * r - q) / w; }
  if ((isz(sp) || sp > 0.f) && (isz(sp - 1.f) || sp < 1.f) && (isz(tp) || tp > 0.f) && (isz(tp - 1.f) || tp < 1.f) &&
      (isz(tp + sp - 1.f) || tp + sp < 1.f)) {
    wit[0] = x0[0] + sp * d1[0] + tp * d2[0]; wit[1] = x0[1] + sp * d1[1] + tp * d2[1]; wit[2] = x0[2] + sp * d1[2] + tp * d2[2];
    bw[0] = 1.f - sp - tp; bw[1] = sp; bw[2] = tp;
    return dot3(wit, wit);
  }
  float w1[3], w2[3], w3[3], t1, t2, t3;
  float e1 = seg_origin(x0, B, w1, &t1), e2 = seg_origin(x0, C, w2, &t2), e3 = seg_origin(B, C, w3, &t3);
  float best = e1; wit[0] = w1[0]; wit[1] = w1[1]; wit[2] = w1[2]; bw[0] = 1.f - t1; bw[1] = t1; bw[2] = 0.f;
  if (e2 < best) { best = e2; wit[0] = w2[0]; wit[1] = w2[1]; wit[2] = w2[2]; bw[0] = 1.f - t2; bw[1] = 0.f; bw[2] = t2; }
  if (e3 < best) { best = e3; wit[0] = w3[0]; wit[1] = w3[1]; wit[2] = w3[2]; bw[0] = 0.f; bw[1] = 1.f - t3; bw[2] = t3; }
  return best;
}

#define MVCOPY(dst, src) do { _Pragma("unroll") for (int _i = 0; _i < 3; _i++) { (dst).v[_i] = (src).v[_i]; (dst).a[_i] = (src).a[_i]; (dst).b[_i] = (src).b[_i]; } } while (0)

// Interior point of a geom for the MPR origin ray.  For primitives it is the point of the primitive closest to
// `target` (the other geom's centre), pulled slightly inside, so that the ray follows the local penetration
// direction: with the fixed geometric centre of a large flat box (the 1.0 x 0.8 m table top) the ray is nearly
// parallel to the contact face and MPR's depth estimate becomes erratic (EPA, which mujoco >= 3.3 uses, has no such
// dependence).  Hulls keep their centre of mass.
DEV void interior_point(const GeomW& G, const float* target, float* out) {
  if (G.type == G_MESH || G.type == G_SPHERE || G.type == G_PLANE) { out[0] = G.c[0]; out[1] = G.c[1]; out[2] = G.c[2]; return; }
  float rel[3] = {target[0] - G.p[0], target[1] - G.p[1], target[2] - G.p[2]}, t[3];
  matTvec3(t, G.R, rel);
  if (G.type == G_BOX) {
#pragma unroll
    for (int i = 0; i < 3; i++) { float lim = G.size[i] - fminf(1e-3f, 0.5f * G.size[i]); t[i] = fminf(fmaxf(t[i], -lim), lim); }
  } else if (G.type == G_CYLINDER) {
    float rmax = G.size[0] - fminf(1e-3f, 0.5f * G.size[0]), rho = sqrtf(t[0] * t[0] + t[1] * t[1]);
    if (rho > rmax) { float sc = rmax / rho; t[0] *= sc; t[1] *= sc; }
    float lim = G.size[1] - fminf(1e-3f, 0.5f * G.size[1]);
    t[2] = fminf(fmaxf(t[2], -lim), lim);
  } else {            // capsule: closest point of the axis segment
    t[0] = 0.f; t[1] = 0.f; t[2] = fminf(fmaxf(t[2], -G.size[1]), G.size[1]);
  }
  float w[3]; matvec3(w, G.R, t);
  out[0] = G.p[0] + w[0]; out[1] = G.p[1] + w[1]; out[2] = G.p[2] + w[2];
}

// EPA (expanding polytope) from the tetrahedron the MPR query ends with - its interior point v0 and the portal v1 v2 v3, which
// contains the origin: the face nearest to the origin is pushed out along its normal until the support point in that direction lies on
// it.  That face is a face of the Minkowski difference and its distance the MINIMUM translation separating the geoms - what mujoco >=
// 3.3's native GJK / EPA reports (the reference enables multiccd on top, so100_task.py:151); MPR's portal is only some face of an inner
// approximation (DESIGN.md section 4 measures the difference against the brute-forced minimum).  Wave-parallel: lane k keeps vertex k
// (with its witness points) and face k (vertex indices, unit normal, distance) in registers, at most 64 of each; one expansion =
// wave-argmin over the faces, one support pair, a visibility ballot, a scan of the visible faces' edges for the horizon, and new faces
// in the freed lanes.  Entirely wave-uniform control flow (G64 policy only).
#define EPA_MAX_EXPANSIONS 30     // 4 + 2 x 30 faces fill the 64 face lanes
struct EpaFace { int a, b, c; float n[3], d; bool alive; };

DEV void epa_make_face(bool doit, int a, int b, int c, float vx, float vy, float vz, EpaFace& F) {
  // (every lane takes part in the exchanges; only `doit` lanes keep the result)
  float A[3] = {wave_bcast_f(vx, a), wave_bcast_f(vy, a), wave_bcast_f(vz, a)};
  float B[3] = {wave_bcast_f(vx, b), wave_bcast_f(vy, b), wave_bcast_f(vz, b)};
  float C[3] = {wave_bcast_f(vx, c), wave_bcast_f(vy, c), wave_bcast_f(vz, c)};
  float e1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, e2[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]}, n[3];
  cross3(n, e1, e2);
  float len = sqrtf(dot3(n, n));
  bool ok = len > 1e-14f;
  float inv = ok ? 1.f / len : 0.f;
  n[0] *= inv; n[1] *= inv; n[2] *= inv;
  float d = dot3(n, A);
  // (no per-face flip: the winding is consistent by construction - the first tetrahedron is oriented as a whole, a new face takes its
  //  horizon edge in the direction the removed face had it - and a per-face sign test turns a face the origin lies ON inside out)
  if (doit) {
    F.a = a; F.b = b; F.c = c;
    F.n[0] = n[0]; F.n[1] = n[1]; F.n[2] = n[2];
    F.d = ok ? d : 3.0e38f; F.alive = ok;
  }
}

template <class Cache, class GP>
DEV bool epa_expand(const DevModel* m, const GeomW& G1, const GeomW& G2, const float* org, const MV& v0, const MV& v1, const MV& v2, const MV& v3,
                    float tol, float* depth, float* dir, float* pos, const Cache& H1, const Cache& H2) {
  __shared__ unsigned int epa_list[WAVE];                 // horizon edges of one expansion, in the order the new faces take them
  int lane = wave_lane();
  float vx = 0.f, vy = 0.f, vz = 0.f, ax = 0.f, ay = 0.f, az = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
#define EPA_PUT(k, X) if (lane == (k)) { vx = X.v[0]; vy = X.v[1]; vz = X.v[2]; ax = X.a[0]; ay = X.a[1]; az = X.a[2]; bx = X.b[0]; by = X.b[1]; bz = X.b[2]; }
  EPA_PUT(0, v0) EPA_PUT(1, v1) EPA_PUT(2, v2) EPA_PUT(3, v3)
  int nv = 4, nf = 4;
  EpaFace F; F.a = F.b = F.c = 0; F.n[0] = F.n[1] = F.n[2] = 0.f; F.d = 3.0e38f; F.alive = false;
  {
    // faces (1 2 3), (0 2 1), (0 3 2), (0 1 3): consistently wound; outward when (v2 - v1) x (v3 - v1) points away from v0, else all four swapped
    float e1[3] = {v2.v[0] - v1.v[0], v2.v[1] - v1.v[1], v2.v[2] - v1.v[2]}, e2[3] = {v3.v[0] - v1.v[0], v3.v[1] - v1.v[1], v3.v[2] - v1.v[2]}, nn[3];
    cross3(nn, e1, e2);
    float to0[3] = {v0.v[0] - v1.v[0], v0.v[1] - v1.v[1], v0.v[2] - v1.v[2]};
    bool swap = dot3(nn, to0) > 0.f;
    int a0 = lane == 0 ? 1 : 0, b0 = lane == 0 ? 2 : (lane == 1 ? 2 : (lane == 2 ? 3 : 1)), c0 = lane == 0 ? 3 : (lane == 1 ? 1 : (lane == 2 ? 2 : 3));
    epa_make_face(lane < 4, lane < 4 ? a0 : 0, lane < 4 ? (swap ? c0 : b0) : 0, lane < 4 ? (swap ? b0 : c0) : 0, vx, vy, vz, F);
  }
  int best = 0; float bd = 0.f, bn[3] = {0.f, 0.f, 0.f};
  bool converged = false;
  for (int it = 0; it <= EPA_MAX_EXPANSIONS; it++) {
    float key = F.alive ? -F.d : -3.0e38f; int idx = lane;
    wave_argmax(key, idx);
    if (key <= -3.0e38f) return false;
    best = idx; bd = -key;
    bn[0] = wave_get_f(F.n[0], best); bn[1] = wave_get_f(F.n[1], best); bn[2] = wave_get_f(F.n[2], best);
    MV w;
    mdsupport<Cache, GP>(m, G1, G2, bn, org, w, H1, H2);
    float reach = dot3(bn, w.v) - bd;
    bool dup = lane < nv && fabsf(vx - w.v[0]) + fabsf(vy - w.v[1]) + fabsf(vz - w.v[2]) < 1e-9f;
#ifdef SO101_EPA_TRACE
    { bool anydup = wave_ballot(dup) != 0ull; if (lane == 0) fprintf(stderr, "  epa it %d best %d bd %.7g reach %.3g nv %d nf %d dup %d w %.6f %.6f %.6f\n", it, best, bd, reach, nv, nf, (int)anydup, w.v[0], w.v[1], w.v[2]); }
#endif
    if (reach <= tol) { converged = true; break; }
    // (a support point the polytope already has, although the face claims room beyond it: rounding has made the polytope inconsistent)
    if (wave_ballot(dup) != 0ull || it == EPA_MAX_EXPANSIONS || nv >= WAVE || nf + 2 > WAVE) break;
    int wi = nv;
    EPA_PUT(wi, w)
    nv++;
    bool vis = F.alive && (F.n[0] * w.v[0] + F.n[1] * w.v[1] + F.n[2] * w.v[2] - F.d > 0.f);
    unsigned long long vmask = wave_ballot(vis);
    int nvis = __popcll(vmask);
    int packed = F.a | (F.b << 8) | (F.c << 16) | ((vis ? 1 : 0) << 24);
    // horizon: an edge of a visible face whose reversed edge belongs to no other visible face
    bool s0 = false, s1 = false, s2 = false;
    for (unsigned long long rest = vmask; rest != 0ull; rest &= rest - 1ull) {      // the visible faces only (a handful of the polytope's)
      int j = (int)__builtin_ctzll(rest);
      int pj = wave_get_i(packed, j);                     // (v_readlane: j is wave-uniform)
      int ja = pj & 255, jb = (pj >> 8) & 255, jc = (pj >> 16) & 255;
#define EPA_REV(x, y) ((ja == (y) && jb == (x)) || (jb == (y) && jc == (x)) || (jc == (y) && ja == (x)))
      bool other = j != lane;
      s0 = s0 || (other && EPA_REV(F.a, F.b)); s1 = s1 || (other && EPA_REV(F.b, F.c)); s2 = s2 || (other && EPA_REV(F.c, F.a));
    }
    bool h0 = vis && !s0, h1 = vis && !s1, h2 = vis && !s2;
    unsigned long long m0 = wave_ballot(h0), m1 = wave_ballot(h1), m2 = wave_ballot(h2);
    int K = __popcll(m0) + __popcll(m1) + __popcll(m2);
#ifdef SO101_EPA_TRACE
    if (lane == 0) fprintf(stderr, "     nvis %d K %d\n", nvis, K);
#endif
    int base = wave_prefix(m0) + wave_prefix(m1) + wave_prefix(m2);
    wave_sync();
    if (h0) epa_list[base] = (unsigned int)(F.a | (F.b << 8));
    if (h1) epa_list[base + (h0 ? 1 : 0)] = (unsigned int)(F.b | (F.c << 8));
    if (h2) epa_list[base + (h0 ? 1 : 0) + (h1 ? 1 : 0)] = (unsigned int)(F.c | (F.a << 8));
    wave_sync();
    int extra = K > nvis ? K - nvis : 0;
    if (nf + extra > WAVE) extra = WAVE - nf;
    bool fresh = lane >= nf && lane < nf + extra;
    int r = vis ? wave_prefix(vmask) : (nvis + lane - nf);
    bool make = (vis || fresh) && r < K;
    unsigned int e = epa_list[make ? r : 0];
    if (vis) { F.alive = false; F.d = 3.0e38f; }
    epa_make_face(make, make ? (int)(e & 255u) : 0, make ? (int)(e >> 8) : 0, make ? wi : 0, vx, vy, vz, F);
    nf += extra;
  }
#undef EPA_PUT
#undef EPA_REV
  // a polytope that has not reached the surface after EPA_MAX_EXPANSIONS (a 0.6 mm sphere deep inside a mesh: the difference is
  // curved everywhere) is an INNER bound, its nearest face too shallow: the caller falls back to MPR's own answer
  if (!converged) return false;
  *depth = bd; dir[0] = bn[0]; dir[1] = bn[1]; dir[2] = bn[2];
  // Witness face.  A flat facet of the Minkowski difference (an edge against an edge, a face against an edge) is triangulated by the
  // polytope; its triangles are coplanar up to rounding, so WHICH of them has the smallest plane distance is decided by the last bit,
  // and the projection of the origin may lie in a neighbour of the winner (a 6 cm hull edge across the 1 m table edge: the clamped
  // barycentric weights of the wrong sliver put the contact 1.2 cm away).  Among the faces coplanar with the nearest one (plane
  // distance within tol, normal within 1e-5) the witness is therefore interpolated on the one that contains the projection best
  // (largest smallest barycentric weight; lane = face, one pass).  Depth and normal stay those of the nearest face.
  {
    float p0[3] = {bd * bn[0], bd * bn[1], bd * bn[2]};
    float fA[3] = {wave_bcast_f(vx, F.a), wave_bcast_f(vy, F.a), wave_bcast_f(vz, F.a)}, fB[3] = {wave_bcast_f(vx, F.b), wave_bcast_f(vy, F.b), wave_bcast_f(vz, F.b)},
          fC[3] = {wave_bcast_f(vx, F.c), wave_bcast_f(vy, F.c), wave_bcast_f(vz, F.c)};
    float g1[3], g2[3], gp[3];
#pragma unroll
    for (int i = 0; i < 3; i++) { g1[i] = fB[i] - fA[i]; g2[i] = fC[i] - fA[i]; gp[i] = p0[i] - fA[i]; }
    float q11 = dot3(g1, g1), q12 = dot3(g1, g2), q22 = dot3(g2, g2), s1 = dot3(gp, g1), s2 = dot3(gp, g2), qden = q11 * q22 - q12 * q12;
    bool okf = qden > 1e-30f;
    float ub = okf ? (q22 * s1 - q12 * s2) / qden : 0.f, uc = okf ? (q11 * s2 - q12 * s1) / qden : 0.f;
    float score = fminf(1.f - ub - uc, fminf(ub, uc));
    bool elig = F.alive && okf && F.d - bd <= tol && F.n[0] * bn[0] + F.n[1] * bn[1] + F.n[2] * bn[2] >= 1.f - 1e-5f;
    float key = elig ? score : -3.0e38f; int widx = lane;
    wave_argmax(key, widx);
    if (key > -3.0e38f) best = widx;
  }
  int ia = wave_bcast_i(F.a, best), ib = wave_bcast_i(F.b, best), ic = wave_bcast_i(F.c, best);
  float A[3] = {wave_bcast_f(vx, ia), wave_bcast_f(vy, ia), wave_bcast_f(vz, ia)}, B[3] = {wave_bcast_f(vx, ib), wave_bcast_f(vy, ib), wave_bcast_f(vz, ib)},
        C[3] = {wave_bcast_f(vx, ic), wave_bcast_f(vy, ic), wave_bcast_f(vz, ic)};
  float p[3] = {bd * bn[0], bd * bn[1], bd * bn[2]}, e1[3], e2[3], ep[3];
#pragma unroll
  for (int i = 0; i < 3; i++) { e1[i] = B[i] - A[i]; e2[i] = C[i] - A[i]; ep[i] = p[i] - A[i]; }
  float d11 = dot3(e1, e1), d12 = dot3(e1, e2), d22 = dot3(e2, e2), r1 = dot3(ep, e1), r2 = dot3(ep, e2), den = d11 * d22 - d12 * d12;
  float wb = den > 1e-30f ? (d22 * r1 - d12 * r2) / den : 0.f, wc = den > 1e-30f ? (d11 * r2 - d12 * r1) / den : 0.f;
  wb = fminf(fmaxf(wb, 0.f), 1.f); wc = fminf(fmaxf(wc, 0.f), 1.f - wb);
  float wa = 1.f - wb - wc;
  float PA[3] = {wave_bcast_f(ax, ia), wave_bcast_f(ay, ia), wave_bcast_f(az, ia)}, PB[3] = {wave_bcast_f(ax, ib), wave_bcast_f(ay, ib), wave_bcast_f(az, ib)},
        PC[3] = {wave_bcast_f(ax, ic), wave_bcast_f(ay, ic), wave_bcast_f(az, ic)};
  float QA[3] = {wave_bcast_f(bx, ia), wave_bcast_f(by, ia), wave_bcast_f(bz, ia)}, QB[3] = {wave_bcast_f(bx, ib), wave_bcast_f(by, ib), wave_bcast_f(bz, ib)},
        QC[3] = {wave_bcast_f(bx, ic), wave_bcast_f(by, ic), wave_bcast_f(bz, ic)};
#pragma unroll
  for (int i = 0; i < 3; i++) pos[i] = 0.5f * ((wa * PA[i] + wb * PB[i] + wc * PC[i]) + (wa * QA[i] + wb * QB[i] + wc * QC[i])) + org[i];
  return true;
}

// MPR penetration query (XenoCollide / libccd ccdMPRPenetration).  Entirely wave-uniform control flow.
template <class Cache, class GP = G64>
DEV bool mpr_penetration(const DevModel* m, const GeomW& G1, const GeomW& G2, float* depth, float* dir, float* pos,
                         const Cache& H1, const Cache& H2) {
  const float mpr_tol = ldc(&m->mpr_tol); const int mpr_iter = ldc(&m->mpr_iter);
  float org[3], c2[3];
  interior_point(G1, G2.c, org);
  interior_point(G2, org, c2);
  MV v0, v1, v2, v3, v4;
#pragma unroll
  for (int i = 0; i < 3; i++) { v0.a[i] = 0.f; v0.b[i] = c2[i] - org[i]; v0.v[i] = -v0.b[i]; }
  if (isz(v0.v[0]) && isz(v0.v[1]) && isz(v0.v[2])) v0.v[0] += 1e-5f;
  float d[3] = {-v0.v[0], -v0.v[1], -v0.v[2]};
  normalize3(d);
  mdsupport<Cache, GP>(m, G1, G2, d, org, v1, H1, H2);
  float dt = dot3(v1.v, d);
  if (isz(dt) || dt < 0.f) return false;
  cross3(d, v0.v, v1.v);
  float dn = sqrtf(dot3(d, d));
  // "origin on the v0-v1 segment": v0 and v1 collinear.  libccd's absolute test |v0 x v1| < eps, with the fp32 epsilon 1.2e-7, fires far from
  // collinearity when the vectors are short - the nudged ray of two coinciding interior points is 1e-5 long, so any support point within 9
  // degrees of it passed for "on the ray" and the pair got the distance to that support point as its depth: a wrist hull whose centre lies
  // inside the static puck reported 76 mm sideways where the minimum translation (and the fp64 oracle, whose epsilon is 1e-10 as in MuJoCo's
  // double-precision build of libccd) says 45 mm through the cap (round 6: seed 3 of test_failure_rates_on_the_headline_workload, env 23;
  // tests/golden/probe_outlier_states.json).  Hence also a RELATIVE bound, sin(angle) < 1e-3: for |v0| |v1| >= 1.2e-4 m^2 - centimetre-sized
  // vectors, every pair whose interior points are apart - the absolute test is the tighter one and decides as before (measured: with 1e-4 the
  // symmetric finger pairs of the ALOHA grippers, whose support points ARE on the ray up to fp32 rounding, went through the full portal search
  // and EPA instead of this exit - the same contacts within the parity tolerances, ALOHA 274 -> 259 k env-steps/s; gpurun_out g16).
  if (dn < fminf(EPS_F, SO101_COLLINEAR_REL * sqrtf(dot3(v0.v, v0.v) * dot3(v1.v, v1.v)))) {
    if (isz(v1.v[0]) && isz(v1.v[1]) && isz(v1.v[2])) {     // touching contact
      *depth = 0.f; dir[0] = dir[1] = dir[2] = 0.f;
#pragma unroll
      for (int i = 0; i < 3; i++) pos[i] = 0.5f * (v1.a[i] + v1.b[i]) + org[i];
      return true;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) { pos[i] = 0.5f * (v1.a[i] + v1.b[i]) + org[i]; dir[i] = v1.v[i]; }
    *depth = normalize3(dir);                                 // origin on the v0-v1 segment
    return true;
  }
  normalize3(d);
  mdsupport<Cache, GP>(m, G1, G2, d, org, v2, H1, H2);
  dt = dot3(v2.v, d);
  if (isz(dt) || dt < 0.f) return false;
  float va[3], vb[3];
#pragma unroll
  for (int i = 0; i < 3; i++) { va[i] = v1.v[i] - v0.v[i]; vb[i] = v2.v[i] - v0.v[i]; }
  cross3(d, va, vb); normalize3(d);
  if (dot3(d, v0.v) > 0.f) {
    MV t; MVCOPY(t, v1); MVCOPY(v1, v2); MVCOPY(v2, t);
    d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2];
  }
  bool have3 = false;
  for (int guard = 0; guard < 100 && !have3; guard++) {
    mdsupport<Cache, GP>(m, G1, G2, d, org, v3, H1, H2);
    dt = dot3(v3.v, d);
    if (isz(dt) || dt < 0.f) return false;
    bool cont = false;
    cross3(va, v1.v, v3.v);
    dt = dot3(va, v0.v);
    if (dt < 0.f && !isz(dt)) { MVCOPY(v2, v3); cont = true; }
    if (!cont) {
      cross3(va, v3.v, v2.v);
      dt = dot3(va, v0.v);
      if (dt < 0.f && !isz(dt)) { MVCOPY(v1, v3); cont = true; }
    }
    if (cont) {
#pragma unroll
      for (int i = 0; i < 3; i++) { va[i] = v1.v[i] - v0.v[i]; vb[i] = v2.v[i] - v0.v[i]; }
      cross3(d, va, vb); normalize3(d);
    } else have3 = true;
  }
  if (!have3) return false;
  // refine the portal until it encloses the origin ray, then push it to the surface
  bool inside = false;
  for (int it = 0; it < 200; it++) {
#pragma unroll
    for (int i = 0; i < 3; i++) { va[i] = v2.v[i] - v1.v[i]; vb[i] = v3.v[i] - v1.v[i]; }
    cross3(d, va, vb); normalize3(d);
    if (!inside) {
      dt = dot3(d, v1.v);
      if (isz(dt) || dt > 0.f) {                                        // portal encapsules origin: start penetration phase
#ifndef SO101_MPR     // (default; -DSO101_MPR = build.py --mpr, libso101_hip_mpr.so, keeps MPR's own answer): EPA takes over here - the tetrahedron v0 v1 v2 v3 contains the
        if constexpr (GP::N == WAVE) {          // origin from now on, and MPR's own refinement of the portal towards the surface is work EPA does anyway
          if constexpr (is_hull_lds<Cache>::value) {
            float* pk = narrow_park_store() + 64;
            if (wave_lane() == 0) {
#pragma unroll
              for (int i = 0; i < 3; i++) { pk[i] = v0.v[i]; pk[3 + i] = v0.a[i]; pk[6 + i] = v0.b[i]; pk[9 + i] = v1.v[i]; pk[12 + i] = v1.a[i]; pk[15 + i] = v1.b[i];
                                            pk[18 + i] = v2.v[i]; pk[21 + i] = v2.a[i]; pk[24 + i] = v2.b[i]; pk[27 + i] = v3.v[i]; pk[30 + i] = v3.a[i]; pk[33 + i] = v3.b[i]; }
            }
            wave_sync();
          }
          if (epa_expand<Cache, GP>(m, G1, G2, org, v0, v1, v2, v3, mpr_tol, depth, dir, pos, H1, H2)) return true;
          if constexpr (is_hull_lds<Cache>::value) {
            wave_sync();
            const float* pk = narrow_park_store() + 64;
#pragma unroll
            for (int i = 0; i < 3; i++) { v0.v[i] = pk[i]; v0.a[i] = pk[3 + i]; v0.b[i] = pk[6 + i]; v1.v[i] = pk[9 + i]; v1.a[i] = pk[12 + i]; v1.b[i] = pk[15 + i];
                                          v2.v[i] = pk[18 + i]; v2.a[i] = pk[21 + i]; v2.b[i] = pk[24 + i]; v3.v[i] = pk[27 + i]; v3.a[i] = pk[30 + i]; v3.b[i] = pk[33 + i]; }
          }
        }
#endif
        inside = true; it = -1; continue;
      }
    }
    mdsupport<Cache, GP>(m, G1, G2, d, org, v4, H1, H2);
    float dv1 = dot3(v1.v, d), dv2 = dot3(v2.v, d), dv3 = dot3(v3.v, d), dv4 = dot3(v4.v, d);
    float dm = fminf(fminf(dv4 - dv1, dv4 - dv2), dv4 - dv3);
    bool reached = isz(dm - mpr_tol) || dm < mpr_tol;
    if (!inside) {
      if (!(isz(dv4) || dv4 > 0.f)) return false;     // cannot encapsule origin
      if (reached || it > 100) return false;
    } else if (reached || it > mpr_iter) {
      float pd[3], bw[3];
      float d2 = origin_tri_dist2(v1.v, v2.v, v3.v, pd, bw);
      *depth = sqrtf(d2);
      if (isz(pd[0]) && isz(pd[1]) && isz(pd[2])) { *depth = 0.f; dir[0] = d[0]; dir[1] = d[1]; dir[2] = d[2]; }
      else { dir[0] = pd[0]; dir[1] = pd[1]; dir[2] = pd[2]; normalize3(dir); }
      // contact position: midpoint of the two witness points of the closest point on the portal (the witness pair
      // GJK/EPA reports); libccd's origin-ray weights are path dependent for deep penetrations
#pragma unroll
      for (int i = 0; i < 3; i++) {
        float p1 = bw[0] * v1.a[i] + bw[1] * v2.a[i] + bw[2] * v3.a[i];
        float p2 = bw[0] * v1.b[i] + bw[1] * v2.b[i] + bw[2] * v3.b[i];
        pos[i] = 0.5f * (p1 + p2) + org[i];
      }
      return true;
    }
    // expand portal
    float v4v0[3]; cross3(v4v0, v4.v, v0.v);
    float t1 = dot3(v1.v, v4v0);
    if (t1 > 0.f) {
      float t2 = dot3(v2.v, v4v0);
      if (t2 > 0.f) MVCOPY(v1, v4); else MVCOPY(v3, v4);
    } else {
      float t3 = dot3(v3.v, v4v0);
      if (t3 > 0.f) MVCOPY(v2, v4); else MVCOPY(v1, v4);
    }
  }
  return false;
}

DEV void make_frame(float* fr) {
  float* x = fr; float* y = fr + 3; float* z = fr + 6;
  y[0] = 0.f; y[1] = 0.f; y[2] = 0.f;
  if (x[1] < 0.5f && x[1] > -0.5f) y[1] = 1.f; else y[2] = 1.f;
  float t = dot3(x, y);
  y[0] -= t * x[0]; y[1] -= t * x[1]; y[2] -= t * x[2];
  normalize3(y);
  cross3(z, x, y);
}

// Upper bound of a hull's support function h(dl) = max_v v . dl (dl: unit direction in the geom frame) from its support-bound table
// (so101_model.hpp DevModel::hull_sbt): bilinear over the four grid points around dl / |dl|_inf on the cube face, times |dl|_inf.
DEV float sbt_bound(const float* T, const float* dl) {
  float a0 = fabsf(dl[0]), a1 = fabsf(dl[1]), a2 = fabsf(dl[2]);
  int ax = a0 >= a1 ? (a0 >= a2 ? 0 : 2) : (a1 >= a2 ? 1 : 2);
  float dm = ax == 0 ? dl[0] : (ax == 1 ? dl[1] : dl[2]);
  float du = ax == 0 ? dl[1] : (ax == 1 ? dl[2] : dl[0]);
  float dv = ax == 0 ? dl[2] : (ax == 1 ? dl[0] : dl[1]);
  float mm = fmaxf(fabsf(dm), 1e-20f), inv = 1.f / mm;
  const float gs = 0.5f * (float)(SBT_GRID - 1);
  float gu = fminf(fmaxf((du * inv + 1.f) * gs, 0.f), (float)(SBT_GRID - 1)), gv = fminf(fmaxf((dv * inv + 1.f) * gs, 0.f), (float)(SBT_GRID - 1));
  int iu = (int)gu; iu = iu > SBT_GRID - 2 ? SBT_GRID - 2 : iu;
  int iv = (int)gv; iv = iv > SBT_GRID - 2 ? SBT_GRID - 2 : iv;
  float fu = gu - (float)iu, fv = gv - (float)iv;
  const float* F = T + ((2 * ax + (dm < 0.f ? 1 : 0)) * SBT_GRID + iu) * SBT_GRID + iv;
  float h = (1.f - fu) * ((1.f - fv) * F[0] + fv * F[1]) + fu * ((1.f - fv) * F[SBT_GRID] + fv * F[SBT_GRID + 1]);
  return h * mm;
}
// lowest extent of mesh geom g (world rotation R, world origin p) along the world unit direction f, from below: min_x (x . f) >= this
DEV float sbt_lowest(const DevModel* m, int g, const float* R, const float* p, const float* f) {
  float dl[3] = {-(R[0] * f[0] + R[3] * f[1] + R[6] * f[2]), -(R[1] * f[0] + R[4] * f[1] + R[7] * f[2]), -(R[2] * f[0] + R[5] * f[1] + R[8] * f[2])};
  return dot3(p, f) - sbt_bound(m->hull_sbt + (size_t)g * SBT_DIM, dl) - 2e-6f;
}

// Round 6: separating directions beyond the oriented boxes' fifteen, for a pair (g1, g2 = a hull) that passed them.  A: world rotation of g1, ca /
// a: centre and half extents of its oriented box, B / cb: the hull's, t = A' (cb - ca).  A third of the candidates that reached the narrowphase
// ended in "no intersection" (3-8 us of a wavefront each): a hull whose ORIENTED BOX dips below a box face although no vertex does, the static puck
// and capsule of the scene under the props' pieces, arm links near props.  The hull's extent along a direction comes from its support-bound
// table - a few per cent of its size above the truth instead of the box's tens of per cent.  Conservative: a pair dropped here has a separating
// plane, so no contact changes (rollouts are bit-identical with and without the tables: scripts/gpu_sbt_ab.py).
DEV bool sbt_separated(const DevModel* m, int g1, int g2, const float* A, const float* ca, const float* a, const float* B, const float* cb, const float* t) {
  const float gap = 1e-6f;
  const int t1 = m->geom_type[g1];
  const float* lc2 = m->geom_aabb + 6 * g2;
  float pb[3];                                 // the hull's geom origin: its box centre minus the rotated local centre
#pragma unroll
  for (int i = 0; i < 3; i++) pb[i] = cb[i] - (B[3 * i] * lc2[0] + B[3 * i + 1] * lc2[1] + B[3 * i + 2] * lc2[2]);
  bool sep = false;
  if (t1 == G_BOX) {
    // the three box faces on the hull's side: the hull's lowest point along the face normal against the face
#pragma unroll
    for (int i = 0; i < 3; i++) {
      float sg = t[i] >= 0.f ? 1.f : -1.f;
      float f[3] = {sg * A[i], sg * A[3 + i], sg * A[6 + i]};
      sep = sep || sbt_lowest(m, g2, B, pb, f) - dot3(ca, f) > a[i] + gap;
    }
    return sep;
  }
  // a sphere / capsule / cylinder / another hull: the centre-to-centre direction, the primitive's axis and the radial direction from that axis
  // as candidate separating directions - the primitive's extent in closed form, a hull's from its table
  const float* lc1 = m->geom_aabb + 6 * g1;
  float pa[3];
#pragma unroll
  for (int i = 0; i < 3; i++) pa[i] = ca[i] - (A[3 * i] * lc1[0] + A[3 * i + 1] * lc1[1] + A[3 * i + 2] * lc1[2]);
  const float r1 = m->geom_size[3 * g1], hl1 = m->geom_size[3 * g1 + 1];
  float az[3] = {A[2], A[5], A[8]};                     // the primitive's axis (capsule, cylinder)
  // highest extent of geom 1 along the unit direction d (world): max_x x . d <= this
  auto top1 = [&](const float* d) -> float {
    float along = fabsf(dot3(az, d));
    if (t1 == G_SPHERE) return dot3(pa, d) + r1;
    if (t1 == G_CAPSULE) return dot3(pa, d) + r1 + hl1 * along;
    if (t1 == G_CYLINDER) return dot3(pa, d) + r1 * sqrtf(fmaxf(1.f - along * along, 0.f)) + hl1 * along;
    float nd[3] = {-d[0], -d[1], -d[2]};
    return -sbt_lowest(m, g1, A, pa, nd);               // (a hull: max x . d = - min x . (-d))
  };
  float dirs[3][3]; int nd_ = 1;
  { float w[3] = {cb[0] - ca[0], cb[1] - ca[1], cb[2] - ca[2]}; float n = sqrtf(dot3(w, w)); float inv = n > 1e-9f ? 1.f / n : 0.f; dirs[0][0] = w[0] * inv; dirs[0][1] = w[1] * inv; dirs[0][2] = w[2] * inv; if (!(n > 1e-9f)) nd_ = 0; }
#pragma unroll
  for (int q = 1; q < 3; q++) { dirs[q][0] = 0.f; dirs[q][1] = 0.f; dirs[q][2] = 0.f; }
  bool has[3] = {nd_ == 1, false, false};
  if (t1 == G_CAPSULE || t1 == G_CYLINDER) {
    float w[3] = {cb[0] - pa[0], cb[1] - pa[1], cb[2] - pa[2]};
    float s_ = dot3(w, az), sg = s_ >= 0.f ? 1.f : -1.f;
    dirs[1][0] = sg * az[0]; dirs[1][1] = sg * az[1]; dirs[1][2] = sg * az[2];
    float rr[3] = {w[0] - s_ * az[0], w[1] - s_ * az[1], w[2] - s_ * az[2]}; float n = sqrtf(dot3(rr, rr)); float inv = n > 1e-9f ? 1.f / n : 0.f;
    dirs[2][0] = rr[0] * inv; dirs[2][1] = rr[1] * inv; dirs[2][2] = rr[2] * inv;
    has[1] = true; has[2] = n > 1e-9f;
  }
#pragma unroll
  for (int q = 0; q < 3; q++)
    if (has[q]) sep = sep || sbt_lowest(m, g2, B, pb, dirs[q]) - top1(dirs[q]) > gap + 2e-6f;
  return sep;
}
// the plane (point pp, unit normal n) against a hull (world rotation B, box centre cb): its lowest point along the normal is above the plane
DEV bool sbt_plane_separated(const DevModel* m, int g2, const float* pp, const float* n, const float* B, const float* cb) {
  const float* lc = m->geom_aabb + 6 * g2;
  float pb[3];
#pragma unroll
  for (int i = 0; i < 3; i++) pb[i] = cb[i] - (B[3 * i] * lc[0] + B[3 * i + 1] * lc[1] + B[3 * i + 2] * lc[2]);
  return sbt_lowest(m, g2, B, pb, n) - dot3(pp, n) > 1e-6f;
}

// ---- multi-contact for flat faces ("multiccd", so101_sim/tasks/base/so100_task.py:151) --------------------------
// MuJoCo's convex-pair multi-contact re-runs the penetration query on configurations tilted by +-1e-3 rad about the
// two tangent axes and keeps results farther apart than 1e-3 of the smaller bounding radius; its native-ccd path
// clips the aligned faces of box / mesh pairs.  Both sample the extreme points of a flat contact patch.  Here that is
// done in closed form whenever one geom presents a flat REFERENCE FACE - the plane, or the box face / cylinder cap along
// which the pair is shallowest (narrow_pair) - and the other (INCIDENT) geom is sampled through its support function:
//   a_0 = support(-f), a_k = support(-f + eps s_k), s_k = (+-u +- v)/sqrt(2) along the face axes, eps = 1e-3.
// A sample becomes a contact when it is below the face plane, inside the face rectangle / disc and farther than
// 1e-3 min(rbound) from the contacts already accepted; all contacts of the pair share the normal +-f.  When a_0 does
// not qualify, the single MPR contact stays.  Other convex pairs keep one contact.  The supports are wave-parallel,
// the control flow is wave-uniform.  (The test oracle restates the same rule in fp64.)
#define FACE_DEPTH_REL 1e-2f
#define FACE_DEPTH_ABS 1e-6f
#define PATCH_EPS 1e-3f
#define PATCH_DUP 1e-3f

// The five sample points of a flat contact patch in ONE pass over the hull: a_0 = support(-f) and
// a_k = support(-f + eps s_k), s_k = (+-u +- v)/sqrt(2) (see face_patch).  Five separate support calls scan a hull five
// times; the banana's hulls have a thousand vertices, more than the register cache holds, so each scan went back to L2
// twice.  Here every vertex is read once and scored against the five directions; the five winners (max dot, smallest
// index - the same vertex support() would return) are fetched afterwards.
struct Patch5 { float p[NCPP][3]; };

// support points of G in NCPP world directions d[k] (unit), one pass over the hull
template <class Cache, class GP = G64>
DEV void support_multi(const DevModel* m, const GeomW& G, const float (*d)[3], Patch5& P, const Cache& H);

template <class Cache, class GP = G64>
DEV void support_patch(const DevModel* m, const GeomW& G, const float* f, const float* u, const float* v, Patch5& P, const Cache& H) {
  float d[NCPP][3];
#pragma unroll
  for (int k = 0; k < NCPP; k++) {
    float su = (k == 1 || k == 4) ? 1.f : -1.f, sv = (k == 1 || k == 2) ? 1.f : -1.f;
    float e = k == 0 ? 0.f : PATCH_EPS * 0.70710678f;
#pragma unroll
    for (int i = 0; i < 3; i++) d[k][i] = -f[i] + e * (su * u[i] + sv * v[i]);
    normalize3(d[k]);
  }
  support_multi<Cache, GP>(m, G, d, P, H);
}

template <class Cache, class GP>
DEV void support_multi(const DevModel* m, const GeomW& G, const float (*d)[3], Patch5& P, const Cache& H) {
  if (G.type != G_MESH) {
#pragma unroll
    for (int k = 0; k < NCPP; k++) support<Cache, GP>(m, G, d[k], P.p[k], H);
    return;
  }
  float dl[NCPP][3], best[NCPP];
  int bi[NCPP];
#pragma unroll
  for (int k = 0; k < NCPP; k++) { matTvec3(dl[k], G.R, d[k]); best[k] = -3.0e38f; bi[k] = 0x7fffffff; }
  int lane = GP::sub();
  const float* x = ldc(&m->vx) + G.vadr; const float* y = ldc(&m->vy) + G.vadr; const float* z = ldc(&m->vz) + G.vadr;
  int first = lane;
  if constexpr (is_hull_sub<Cache>::value) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
      int i = H.i[q];
#pragma unroll
      for (int k = 0; k < NCPP; k++) {
        float s = H.x[q] * dl[k][0] + H.y[q] * dl[k][1] + H.z[q] * dl[k][2];
        if (i < G.vnum && s > best[k]) { best[k] = s; bi[k] = i; }
      }
    }
    first = G.vnum;
  } else if constexpr (is_hull_lds<Cache>::value) {
    const float4* X4 = (const float4*)H.p; const float4* Y4 = (const float4*)(H.p + H.n); const float4* Z4 = (const float4*)(H.p + 2 * H.n);
    auto block = [&](int J) {
      float4 xv = X4[GP::N * J + lane], yv = Y4[GP::N * J + lane], zv = Z4[GP::N * J + lane];
      float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ys[4] = {yv.x, yv.y, yv.z, yv.w}, zs[4] = {zv.x, zv.y, zv.z, zv.w};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        int i = 4 * GP::N * J + 4 * lane + q;
#pragma unroll
        for (int k = 0; k < NCPP; k++) {
          float s = xs[q] * dl[k][0] + ys[q] * dl[k][1] + zs[q] * dl[k][2];
          if (i < G.vnum && s > best[k]) { best[k] = s; bi[k] = i; }
        }
      }
    };
    if constexpr (GP::N == WAVE) {
#pragma unroll
      for (int J = 0; J < HULL_LDS_MAX / (4 * WAVE); J++) {
        if (4 * WAVE * J >= G.vnum || 4 * WAVE * J >= H.n) break;
        block(J);
      }
    } else {
      const int lim = G.vnum < H.n ? G.vnum : H.n;
#pragma unroll 1
      for (int J = 0; 4 * GP::N * J < lim; J++) block(J);
    }
    first = lane + H.n;
  } else if constexpr (sizeof(Cache) >= sizeof(HullCache)) {
#pragma unroll
    for (int j = 0; j < HULL_K; j++) {
      if (GP::N * j >= G.vnum) break;
      int i = lane + GP::N * j;
      float X = H.x[j], Y = H.y[j], Z = H.z[j];
#pragma unroll
      for (int k = 0; k < NCPP; k++) {
        float s = X * dl[k][0] + Y * dl[k][1] + Z * dl[k][2];
        if (i < G.vnum && s > best[k]) { best[k] = s; bi[k] = i; }
      }
    }
    first = lane + GP::N * HULL_K;
  }
#pragma unroll 4
  for (int i = first; i < G.vnum; i += GP::N) {
    float X = x[i], Y = y[i], Z = z[i];
#pragma unroll
    for (int k = 0; k < NCPP; k++) {
      float s = X * dl[k][0] + Y * dl[k][1] + Z * dl[k][2];
      if (s > best[k]) { best[k] = s; bi[k] = i; }
    }
  }
  // the five reductions first, then the five winners' coordinates in one burst of loads (fetching each winner right
  // after its reduction put five L2 round trips in series), then the transforms
#pragma unroll
  for (int k = 0; k < NCPP; k++) { if constexpr (is_hull_sub<Cache>::value) GP::argmax_lean(best[k], bi[k]); else GP::argmax(best[k], bi[k]); }
  float loc[NCPP][3];
#pragma unroll
  for (int k = 0; k < NCPP; k++) {
    int w = (unsigned int)bi[k] < (unsigned int)G.vnum ? bi[k] : 0;       // (a non-finite direction selects nothing)
    if constexpr (is_hull_lds<Cache>::value) {
      if (w < H.n) { loc[k][0] = H.p[w]; loc[k][1] = H.p[H.n + w]; loc[k][2] = H.p[2 * H.n + w]; continue; }      // (the staged copy: same floats)
    }
    loc[k][0] = x[w]; loc[k][1] = y[w]; loc[k][2] = z[w];
  }
#pragma unroll
  for (int k = 0; k < NCPP; k++) {
    float wv[3];
    matvec3(wv, G.R, loc[k]);
    P.p[k][0] = G.p[0] + wv[0]; P.p[k][1] = G.p[1] + wv[1]; P.p[k][2] = G.p[2] + wv[2];
  }
}

// contacts of one geom pair: slot k holds patch sample k (or the single MPR contact in slot 0) when bit k of `valid` is
// set - fixed slots instead of a compacted list: "store at the running count" is register indexing, i.e. scratch memory
struct PairContacts { unsigned int valid; float nrm[3], dist[NCPP], pos[NCPP][3]; };

// inside the face outline (rectangle hu x hv, or disc of radius hu when hv < 0) by at least `margin`
DEV bool inside_margin(const float* rel, const float* u, const float* v, float hu, float hv, float margin) {
  float pu = dot3(rel, u), pv = dot3(rel, v), ru = hu - margin;
  if (hv >= 0.f) return fabsf(pu) <= ru && fabsf(pv) <= hv - margin;
  return ru >= 0.f && pu * pu + pv * pv <= ru * ru;
}

DEV bool inside_face(const float* rel, const float* u, const float* v, float hu, float hv) {
  if (hu < 0.f) return true;                                          // unbounded plane
  float pu = dot3(rel, u), pv = dot3(rel, v);
  return hv >= 0.f ? (fabsf(pu) <= hu && fabsf(pv) <= hv) : (pu * pu + pv * pv <= hu * hu);      // rectangle / disc
}



DEV bool face_patch(const Patch5& P, const float* f, const float* c, const float* u, const float* v, float hu, float hv,
                    float dup_tol, PairContacts& out) {
  out.valid = 0u;
#pragma unroll
  for (int k = 0; k < NCPP; k++) {
    const float* p = P.p[k];
    float rel[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
    float dist = dot3(rel, f);
    bool ok = dist < 0.f;
    ok = ok && inside_face(rel, u, v, hu, hv);
    if (k == 0 && !ok) return false;
    float cp[3] = {p[0] - 0.5f * dist * f[0], p[1] - 0.5f * dist * f[1], p[2] - 0.5f * dist * f[2]};
#pragma unroll
    for (int j = 0; j < k; j++) {
      float dd[3] = {cp[0] - out.pos[j][0], cp[1] - out.pos[j][1], cp[2] - out.pos[j][2]};
      if (((out.valid >> j) & 1u) && sqrtf(dot3(dd, dd)) < dup_tol) ok = false;
    }
    out.dist[k] = dist; out.pos[k][0] = cp[0]; out.pos[k][1] = cp[1]; out.pos[k][2] = cp[2];
    if (ok) out.valid |= 1u << k;
  }
  return true;
}

// flat face number `axis` of box / cylinder G on the side that `toward` (world, any length) points to (box: local
// x/y/z; cylinder: only axis 2, the cap): outward normal f, centre c, in-plane axes u/v with half extents (hv < 0: disc
// of radius hu).  Returns false when the geom has no such face.
DEV bool flat_face(const GeomW& G, int axis, const float* toward, float* f, float* c, float* u, float* v, float* hu, float* hv, float* half) {
  float loc[3]; matTvec3(loc, G.R, toward);
  if (G.type == G_CYLINDER) {
    if (axis != 2) return false;
    float sg = loc[2] >= 0.f ? 1.f : -1.f;
#pragma unroll
    for (int k = 0; k < 3; k++) { f[k] = sg * G.R[3 * k + 2]; u[k] = G.R[3 * k]; v[k] = G.R[3 * k + 1]; c[k] = G.p[k] + f[k] * G.size[1]; }
    *hu = G.size[0]; *hv = -1.f; *half = G.size[1];
    return true;
  }
  // axis picks as 0/1 weights (exact arithmetic; chains of selects on the index get turned into indexed loads of a
  // stack copy of the geom, i.e. scratch memory)
  float w0 = axis == 0 ? 1.f : 0.f, w1 = axis == 1 ? 1.f : 0.f, w2 = axis == 2 ? 1.f : 0.f;
  float li = w0 * loc[0] + w1 * loc[1] + w2 * loc[2];
  float sg = li >= 0.f ? 1.f : -1.f;
  // u axis = (axis + 1) % 3 -> weights (w2, w0, w1); v axis = (axis + 2) % 3 -> weights (w1, w2, w0)
  float si = w0 * G.size[0] + w1 * G.size[1] + w2 * G.size[2];
  *half = si;
  *hu = w2 * G.size[0] + w0 * G.size[1] + w1 * G.size[2];
  *hv = w1 * G.size[0] + w2 * G.size[1] + w0 * G.size[2];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    f[k] = sg * (w0 * G.R[3 * k] + w1 * G.R[3 * k + 1] + w2 * G.R[3 * k + 2]);
    u[k] = w2 * G.R[3 * k] + w0 * G.R[3 * k + 1] + w1 * G.R[3 * k + 2];
    v[k] = w1 * G.R[3 * k] + w2 * G.R[3 * k + 1] + w0 * G.R[3 * k + 2];
    c[k] = G.p[k] + f[k] * si;
  }
  return true;
}

// The direction (world, not normalised) of the FIRST support query that narrow_pair_cached() makes on the hull G2 of a light pair - the plane's normal
// negated, or the outward normal, negated, of the box face scan_faces() visits first (same expressions as there) - and the cell of G2's support-vertex
// lists it falls into.  Shared by the wavefront that writes the work item and the one that serves it.  -1: no such query (not a plane / box against a hull).
DEV int light_first_cell(const GeomW& G1, const GeomW& G2) {
  if (G2.type != G_MESH) return -1;
  float f[3];
  if (G1.type == G_PLANE) { f[0] = G1.R[2]; f[1] = G1.R[5]; f[2] = G1.R[8]; }
  else if (G1.type == G_BOX) {
    float toward[3] = {G2.c[0] - G1.c[0], G2.c[1] - G1.c[1], G2.c[2] - G1.c[2]};
    float loc[3]; matTvec3(loc, G1.R, toward);
    float lb0 = G1.size[0] - fabsf(loc[0]), lb1 = G1.size[1] - fabsf(loc[1]), lb2 = G1.size[2] - fabsf(loc[2]);
    int axis = 0; float bl = lb0;
    if (lb1 < bl) { axis = 1; bl = lb1; }
    if (lb2 < bl) { axis = 2; bl = lb2; }
    if (!(bl < 3.0e38f)) return -1;                      // (non-finite bounds: the full query)
    float w0 = axis == 0 ? 1.f : 0.f, w1 = axis == 1 ? 1.f : 0.f, w2 = axis == 2 ? 1.f : 0.f;
    float li = w0 * loc[0] + w1 * loc[1] + w2 * loc[2], sg = li >= 0.f ? 1.f : -1.f;
#pragma unroll
    for (int k = 0; k < 3; k++) f[k] = sg * (w0 * G1.R[3 * k] + w1 * G1.R[3 * k + 1] + w2 * G1.R[3 * k + 2]);
  } else return -1;
  float nf[3] = {-f[0], -f[1], -f[2]}, dl[3];
  matTvec3(dl, G2.R, nf);
  if (!(fabsf(dl[0]) + fabsf(dl[1]) + fabsf(dl[2]) > 0.5f)) return -1;      // (a diverged pose)
  return hl_cell(dl);
}

#ifdef SO101_DEBUG_CLOCKS
#define QPROF(k) { unsigned long long qn_ = SO101_CLOCK(); if (prof && wave_lane() == 0) atomicAdd(&prof[k], (unsigned int)(qn_ - qp_)); qp_ = qn_; }
#else
#define QPROF(k)
#endif
struct FaceRef { float f[3], c[3], u[3], v[3], hu, hv, depth; int side; bool exact, separated; Patch5 P; };

// Flat-face scan of GR (box / cylinder) against the incident geom GI, before any iterative query.  For every flat face
// on the side of GI's centre, a0 = GI's deepest point below the face plane, d0 its depth:
//  * d0 <= 0: the face plane separates the pair - no contact, exactly (R.separated);
//  * a0 inside the face outline with a lateral margin >= d0, and d0 <= the half thickness behind the face: a0 is a point
//    of the box at distance d0 from the box's boundary, so no translation shorter than d0 separates the pair and the
//    translation d0 along the face normal does - minimum penetration depth d0 along the face normal, EXACTLY, and no
//    iterative query is needed (R.exact: props resting on the table top, finger pads, the static puck);
//  * a0 merely inside the outline (d0 <= half thickness): a CANDIDATE; the shallowest one is kept in R and later wins
//    over MPR's answer when it is not deeper (narrow_pair).
// ONE_FACE (k_narrow's fast path, HullSub): only the face visited first - the incident hull's subset is valid for that face's normal alone;
// a pair that face does not settle (neither separated nor exact) is handed back to the full query.
template <class Cache, class GP = G64, bool ONE_FACE = false>
DEV void scan_faces(const DevModel* m, const GeomW& GR, const GeomW& GI, const Cache& HI, int side, FaceRef& R, unsigned int* prof = nullptr) {
  if (GR.type != G_BOX && GR.type != G_CYLINDER) return;
#ifdef SO101_DEBUG_CLOCKS
  unsigned long long qp_ = SO101_CLOCK();
#endif
  float toward[3] = {GI.c[0] - GR.c[0], GI.c[1] - GR.c[1], GI.c[2] - GR.c[2]};
  // Visiting order: increasing depth of the incident's centre below the face plane (= half extent along the axis minus
  // |centre offset along it|, a lower bound of d0), i.e. the face the incident geom sticks out of first - for a prop on
  // the table the top face.  The scan ends at the first EXACT face: the geoms then share the point a0, so no other face
  // plane separates them, and another exact face would give the same depth.  (Saves two of three hull scans for every
  // hull resting on the table; the result does not depend on the order otherwise.)
  float loc[3]; matTvec3(loc, GR.R, toward);
  float lb0 = GR.size[0] - fabsf(loc[0]), lb1 = GR.size[1] - fabsf(loc[1]), lb2 = GR.size[2] - fabsf(loc[2]);
  unsigned int done = 0u;
#pragma unroll 1
  for (int it = 0; it < (ONE_FACE ? 1 : 3); it++) {
    if (R.separated || R.exact) break;
    int axis = 0; float bl = 3.0e38f;
    if (!(done & 1u)) { axis = 0; bl = lb0; }
    if (!(done & 2u) && lb1 < bl) { axis = 1; bl = lb1; }
    if (!(done & 4u) && lb2 < bl) { axis = 2; bl = lb2; }
    if (bl == 3.0e38f) axis = (done & 1u) ? ((done & 2u) ? 2 : 1) : 0;          // (non-finite bounds: plain index order)
    done |= 1u << axis;
    float f[3], c[3], u[3], v[3], hu, hv, half;
    if (!flat_face(GR, axis, toward, f, c, u, v, &hu, &hv, &half)) continue;
    float cr[3] = {c[0] - GI.c[0], c[1] - GI.c[1], c[2] - GI.c[2]};
    if (dot3(cr, f) > half) continue;                  // d0 >= depth of the incident's centre > half thickness
    float nf[3] = {-f[0], -f[1], -f[2]}, a0[3];
    QPROF(6)
    support<Cache, GP>(m, GI, nf, a0, HI);
    QPROF(7)
    float rel[3] = {a0[0] - c[0], a0[1] - c[1], a0[2] - c[2]};
    float d0 = -dot3(rel, f);
    if (!(d0 > 0.f)) { R.separated = true; continue; }
    if (d0 > half || !inside_face(rel, u, v, hu, hv)) continue;
    bool ex = inside_margin(rel, u, v, hu, hv, d0);
    if (!ex && !(d0 < R.depth)) continue;
    R.exact = ex; R.depth = d0; R.side = side; R.hu = hu; R.hv = hv;
#pragma unroll
    for (int k = 0; k < 3; k++) { R.f[k] = f[k]; R.c[k] = c[k]; R.u[k] = u[k]; R.v[k] = v[k]; }
    // the face is (so far) the reference face: its five patch samples in one more pass over the incident hull
    // (taking them in the same pass that finds a0 for the face visited first measured no faster: 1.257 M vs 1.261 M
    // env-steps/s at 32768 envs - the passes over the hull are not what a candidate's 5-10 us go into)
    Patch5 P;
    QPROF(8)
    support_patch<Cache, GP>(m, GI, f, u, v, P, HI);
#pragma unroll
    for (int k = 0; k < NCPP; k++) { R.P.p[k][0] = P.p[k][0]; R.P.p[k][1] = P.p[k][1]; R.P.p[k][2] = P.p[k][2]; }
    QPROF(9)
  }
}

// Hull against hull (round 5; the reference runs with multiccd, so100_task.py:151, aloha2_task.py:197): behind the EPA contact (slot 0) the
// extreme points of whatever flat feature each hull presents along the contact normal n (geom 1 -> geom 2).  With w1 = pos + depth/2 n on
// geom 1's surface and w2 = pos - depth/2 n on geom 2's:
//   b_k = support_2(-n + eps s_k), a_k = support_1(+n + eps s_k), k = 1..4 (the tilted samples of support_patch);
//   b_k is a contact when it lies below geom 1's supporting plane (through w1) and, with r the unit lateral direction from w1 to b_k,
//   r . (b_k - w1) <= r . (support_1(n + eps r) - w1) + 1e-6 - inside the extent of geom 1's feature in that direction, again by a tilted
//   support (a vertex or a curved patch has extent 0: nothing beyond the EPA contact survives); samples laterally closer than dup_tol to
//   w1 are skipped (they would repeat the EPA contact); a_k likewise against geom 2 at w2.
// Accepted in the order b_1..b_4, a_1..a_4 while farther than dup_tol from those already accepted, NCPP in all; normal n for all, distance
// = the sample's signed distance to the other hull's plane, position = the midpoint.  Four more passes over the hulls (two of samples, two
// of extents), only for mesh pairs that EPA found in contact.  (The test suite holds an fp64 restatement of the rule.)
template <class Cache, class GP = G64>
DEV void hull_patch(const DevModel* m, const GeomW& G1, const GeomW& G2, const Cache& H1, const Cache& H2, const float* n, float depth, const float* pos,
                    float dup_tol, PairContacts& out) {
  float fr[9] = {n[0], n[1], n[2], 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  make_frame(fr);
  const float* u = fr + 3; const float* v = fr + 6;
  float nn[3] = {-n[0], -n[1], -n[2]};
  float w1[3], w2[3];
#pragma unroll
  for (int i = 0; i < 3; i++) { w1[i] = pos[i] + 0.5f * depth * n[i]; w2[i] = pos[i] - 0.5f * depth * n[i]; }
  int count = 1;                                       // (slot 0: the EPA contact, already in `out`)
#pragma unroll 1
  for (int side = 0; side < 2; side++) {
    if (count >= NCPP) break;
    const float sg = side == 0 ? -1.f : 1.f;
    GeomW GS, GO; Cache HS, HO;
    select_geom(side == 0, G2, G1, GS); select_geom(side == 0, G1, G2, GO);
    select_hull(side == 0, H2, H1, HS); select_hull(side == 0, H1, H2, HO);
    float wo[3] = {side == 0 ? w1[0] : w2[0], side == 0 ? w1[1] : w2[1], side == 0 ? w1[2] : w2[2]};
    Patch5 S;
    support_patch<Cache, GP>(m, GS, side == 0 ? n : nn, u, v, S, HS);        // slots 1..4: support(sg n + eps s_k)
    float dist[4], rl[4], de[NCPP][3], r[4][3];
    bool cand[4];
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float* p = S.p[k + 1];
      float rel[3] = {p[0] - wo[0], p[1] - wo[1], p[2] - wo[2]};
      float h = dot3(rel, n);
      dist[k] = -sg * h;
      cand[k] = dist[k] < 0.f;
      r[k][0] = rel[0] - h * n[0]; r[k][1] = rel[1] - h * n[1]; r[k][2] = rel[2] - h * n[2];
      rl[k] = normalize3(r[k]);
      // (a sample laterally closer than dup_tol to the EPA witness would only repeat the EPA contact: a vertex or an edge end - skipped
      //  before the extent pass, which is then not run at all for a hull that presents a vertex)
      cand[k] = cand[k] && rl[k] >= dup_tol;
      bool ext = cand[k];
      any = any || ext;
#pragma unroll
      for (int i = 0; i < 3; i++) de[k + 1][i] = ext ? -sg * n[i] + PATCH_EPS * r[k][i] : -sg * n[i];
      normalize3(de[k + 1]);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) de[0][i] = -sg * n[i];
    Patch5 E;
#pragma unroll
    for (int k = 0; k < NCPP; k++) { E.p[k][0] = wo[0]; E.p[k][1] = wo[1]; E.p[k][2] = wo[2]; }
    if (any) support_multi<Cache, GP>(m, GO, de, E, HO);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      bool ok = cand[k] && count < NCPP;
      if (ok) {
        const float* e = E.p[k + 1];
        float ext = r[k][0] * (e[0] - wo[0]) + r[k][1] * (e[1] - wo[1]) + r[k][2] * (e[2] - wo[2]);
        ok = rl[k] <= ext + 1e-6f;
      }
      const float* p = S.p[k + 1];
      float cp[3] = {p[0] + sg * 0.5f * dist[k] * n[0], p[1] + sg * 0.5f * dist[k] * n[1], p[2] + sg * 0.5f * dist[k] * n[2]};
#pragma unroll
      for (int j = 0; j < NCPP; j++) {
        float dd[3] = {cp[0] - out.pos[j][0], cp[1] - out.pos[j][1], cp[2] - out.pos[j][2]};
        if (((out.valid >> j) & 1u) && sqrtf(dot3(dd, dd)) < dup_tol) ok = false;
      }
      if (ok) {
#pragma unroll
        for (int t = 1; t < NCPP; t++)                 // (slot = count: selects instead of a dynamic register index)
          if (count == t) { out.dist[t] = dist[k]; out.pos[t][0] = cp[0]; out.pos[t][1] = cp[1]; out.pos[t][2] = cp[2]; }
        out.valid |= 1u << count;
        count++;
      }
    }
  }
}

// Narrowphase of one candidate pair (geom types ordered): up to NCPP contacts sharing one normal (geom1 -> geom2),
// each with its penetration distance (< 0) and position.
// narrow_pair_cached: the caches H1 / H2 are ready (k_narrow stages them in LDS), rb1 / rb2 = the geoms' bounding radii
// FACES_ONLY (k_narrow's row pass, policy G16: four pairs per wavefront, one per DPP row): the plane and flat-face closed forms only; returns
// false when the pair needs the iterative query (MPR / EPA), which the caller then runs with the whole wavefront.  Otherwise returns true.
template <class Cache, class GP = G64, bool FACES_ONLY = false, bool ONE_FACE = false>
DEV bool narrow_pair_cached(const DevModel* m, const GeomW& G1, const GeomW& G2, float rb1, float rb2, const Cache& H1, const Cache& H2, PairContacts& out,
                            unsigned int* prof = nullptr) {
  static_assert(!ONE_FACE || FACES_ONLY, "the one-face scan has no iterative query behind it");
#ifdef SO101_DEBUG_CLOCKS
  unsigned long long qp_ = SO101_CLOCK();
#endif
  out.valid = 0u; out.nrm[0] = out.nrm[1] = out.nrm[2] = 0.f;
#pragma unroll
  for (int j = 0; j < NCPP; j++) { out.dist[j] = 0.f; out.pos[j][0] = out.pos[j][1] = out.pos[j][2] = 0.f; }
  if (G1.type == G_PLANE) {
    float fr[9] = {G1.R[2], G1.R[5], G1.R[8], 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    make_frame(fr);
    Patch5 P;
    support_patch<Cache, GP>(m, G2, fr, fr + 3, fr + 6, P, H2);
    face_patch(P, fr, G1.p, fr + 3, fr + 6, -1.f, -1.f, PATCH_DUP * rb2, out);
    out.nrm[0] = fr[0]; out.nrm[1] = fr[1]; out.nrm[2] = fr[2];
    return true;
  }
  FaceRef best;
  best.depth = 3.0e38f; best.side = -1; best.hu = 0.f; best.hv = 0.f; best.exact = false; best.separated = false;
#pragma unroll
  for (int k = 0; k < 3; k++) { best.f[k] = 0.f; best.c[k] = 0.f; best.u[k] = 0.f; best.v[k] = 0.f; }
#pragma unroll
  for (int k = 0; k < NCPP; k++) { best.P.p[k][0] = 0.f; best.P.p[k][1] = 0.f; best.P.p[k][2] = 0.f; }
  scan_faces<Cache, GP, ONE_FACE>(m, G1, G2, H2, 0, best, prof);
  if constexpr (!ONE_FACE) { if (!best.separated && !best.exact) scan_faces<Cache, GP>(m, G2, G1, H1, 1, best, prof); }
  QPROF(2)
  if (best.separated) return true;
  float depth = 0.f, nrm[3] = {0.f, 0.f, 0.f}, pos[3] = {0.f, 0.f, 0.f};
  if constexpr (FACES_ONLY) { if (!best.exact) return false; }
  else if (!best.exact) {
    if constexpr (is_hull_lds<Cache>::value) {
      float* pk = narrow_park_store();
      if (wave_lane() == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) { pk[k] = best.f[k]; pk[3 + k] = best.c[k]; pk[6 + k] = best.u[k]; pk[9 + k] = best.v[k]; }
        pk[12] = best.hu; pk[13] = best.hv; pk[14] = best.depth; pk[15] = __int_as_float(best.side);
#pragma unroll
        for (int k = 0; k < NCPP; k++) { pk[16 + 3 * k] = best.P.p[k][0]; pk[17 + 3 * k] = best.P.p[k][1]; pk[18 + 3 * k] = best.P.p[k][2]; }
      }
      wave_sync();
    }
    // MPR's depth is the depth along ITS final portal normal, which for a thin plate (finger pad) against a hull can be
    // an oblique direction ten times deeper than the plate's face normal: the shallowest face candidate wins when it
    // is not deeper (1 % + 1e-6 m slack: for a face contact both are the same number)
    bool ok = mpr_penetration<Cache, GP>(m, G1, G2, &depth, nrm, pos, H1, H2);
    if (!ok || !(depth > 0.f)) return true;
    if constexpr (is_hull_lds<Cache>::value) {
      wave_sync();
      const float* pk = narrow_park_store();
#pragma unroll
      for (int k = 0; k < 3; k++) { best.f[k] = pk[k]; best.c[k] = pk[3 + k]; best.u[k] = pk[6 + k]; best.v[k] = pk[9 + k]; }
      best.hu = pk[12]; best.hv = pk[13]; best.depth = pk[14]; best.side = __float_as_int(pk[15]);
#pragma unroll
      for (int k = 0; k < NCPP; k++) { best.P.p[k][0] = pk[16 + 3 * k]; best.P.p[k][1] = pk[17 + 3 * k]; best.P.p[k][2] = pk[18 + 3 * k]; }
    }
    if (best.side >= 0 && !(best.depth <= depth * (1.f + FACE_DEPTH_REL) + FACE_DEPTH_ABS)) best.side = -1;
  }
  QPROF(3)
  int ref = best.side;
  bool patched = false;
  if (ref >= 0) patched = face_patch(best.P, best.f, best.c, best.u, best.v, best.hu, best.hv, PATCH_DUP * fminf(rb1, rb2), out);
  QPROF(13)
  const float* f = best.f;
  if (patched) {
    float sg = ref == 0 ? 1.f : -1.f;
    out.nrm[0] = sg * f[0]; out.nrm[1] = sg * f[1]; out.nrm[2] = sg * f[2];
  } else if (best.exact) {
    out.valid = 0u;
  } else {
    out.valid = 1u; out.dist[0] = -depth;
#pragma unroll
    for (int k = 0; k < 3; k++) { out.nrm[k] = nrm[k]; out.pos[0][k] = pos[k]; }
#if !defined(SO101_NO_HULL_PATCH) && !defined(SO101_MPR)      // (the MPR option keeps the single contact: its portal normal is no face normal of the Minkowski difference; NO_HULL_PATCH: kernel experiments)
    if constexpr (!FACES_ONLY) {
      // (inlined.  Measured in k_narrow, round 5, env-steps/s at 4096 envs: at three wavefronts per SIMD the patch code costs 96 more spilled
      //  VGPRs on the common path - 656 k against 738 k without it -, out of line behind a call with its arguments in LDS 537 k; at two
      //  wavefronts per SIMD nothing spills: 730 k)
      if (G1.type == G_MESH && G2.type == G_MESH) hull_patch<Cache, GP>(m, G1, G2, H1, H2, nrm, depth, pos, PATCH_DUP * fminf(rb1, rb2), out);
    }
#endif
  }
  QPROF(14)
  return true;
}

template <class Cache, class GP = G64>
DEV void narrow_pair(const DevModel* m, const GeomW& G1, const GeomW& G2, int g1, int g2, PairContacts& out, unsigned int* prof = nullptr) {
  static_assert(!is_hull_lds<Cache>::value, "the LDS cache is staged by its kernel: narrow_pair_cached");
#ifdef SO101_DEBUG_CLOCKS
  unsigned long long qp_ = SO101_CLOCK();
#endif
  Cache H1, H2;
  hull_load<GP>(m, G1, H1); hull_load<GP>(m, G2, H2);
  QPROF(1)
  float rb1 = GP::ld(ldc(&m->geom_rbound) + g1), rb2 = GP::ld(ldc(&m->geom_rbound) + g2);
  narrow_pair_cached<Cache, GP>(m, G1, G2, rb1, rb2, H1, H2, out, prof);
}
