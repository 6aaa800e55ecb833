// TEST HARNESS ONLY - device probes of the hull support queries of so101_geom.hpp, for tests/test_support_queries.py.
// tests/devprims/__init__.py builds this file with hipcc for gfx950 (the product's flags, so101_sim_amd/build.py FLAGS) or with g++ against the
// lane-thread emulation of tests/hostemu.  The product never links it (so101_sim_amd/build.py compiles csrc/*.hip only).
// One hull per handle: a mesh geom at the origin with the identity rotation, so that a support point is a vertex, float for float.  Support
// queries run one per 64-lane workgroup (G16: four per workgroup, one per row of 16 lanes); the pure functions run one per lane.
#include <hip/hip_runtime.h>
#ifdef SO101_EMU
thread_local emu_idx threadIdx;
thread_local emu_idx blockIdx;
thread_local EmuBlock* emu_blk;
#endif
#include "../../so101_sim_amd/csrc/so101_geom.hpp"
#include "../../so101_sim_amd/csrc/so101_tables.hpp"

#include <cmath>
#include <vector>

// support paths (tests/devprims/__init__.py PATHS): the cache and lane-group policy combinations the product runs
enum { P_NOCACHE = 0, P_HULLCACHE = 1, P_LDS = 2, P_LDS_G16 = 3, P_SUB = 4, P_COUNT };
#define GEOM_WORDS 19      // packed GeomW of probe_first_cell: type, size[3], R[9], p[3], c[3]

namespace {

DEV void probe_geom(int vnum, GeomW& G) {
  G.type = G_MESH; G.vadr = 0; G.vnum = vnum;
#pragma unroll
  for (int i = 0; i < 3; i++) { G.size[i] = 0.f; G.p[i] = 0.f; G.c[i] = 0.f; }
#pragma unroll
  for (int i = 0; i < 9; i++) G.R[i] = i % 4 == 0 ? 1.f : 0.f;
}

// query i: a direction (3 floats) or a patch frame f | u | v (9); result: the support point (3) or the patch's NCPP points (3 NCPP)
template <class Cache, class GP>
DEV void probe_one(const DevModel* m, const GeomW& G, int patch, const float* qs, int i, float* out, bool write, const Cache& H) {
  float q[9];
  const int qw = patch ? 9 : 3;
#pragma unroll
  for (int k = 0; k < 9; k++) q[k] = k < qw ? qs[qw * i + k] : 0.f;
  if (patch) {
    Patch5 P;
    support_patch<Cache, GP>(m, G, q, q + 3, q + 6, P, H);
    if (write)
      for (int k = 0; k < NCPP; k++) for (int j = 0; j < 3; j++) out[3 * NCPP * i + 3 * k + j] = P.p[k][j];
  } else {
    float o[3];
    support<Cache, GP>(m, G, q, o, H);
    if (write) for (int j = 0; j < 3; j++) out[3 * i + j] = o[j];
  }
}

template <int PATH>
__global__ __launch_bounds__(64) void k_support(const DevModel* m, int vnum, int nslots, int patch, const float* qs, const int* cells, int nq, int nblk, float* out) {
  __shared__ __attribute__((aligned(16))) float pool[3 * HULL_LDS_MAX];
  const int lane = wave_lane();
  GeomW G; probe_geom(vnum, G);
  if constexpr (PATH == P_NOCACHE) {
    NoCache H;
    for (int i = blockIdx.x; i < nq; i += nblk) probe_one<NoCache, G64>(m, G, patch, qs, i, out, lane == 0, H);
  } else if constexpr (PATH == P_HULLCACHE) {
    HullCache H; hull_load<G64>(m, G, H);
    for (int i = blockIdx.x; i < nq; i += nblk) probe_one<HullCache, G64>(m, G, patch, qs, i, out, lane == 0, H);
  } else if constexpr (PATH == P_LDS) {
    HullLDS H{pool, nslots};
    hull_load<G64>(m, G, H);
    wave_sync();
    for (int i = blockIdx.x; i < nq; i += nblk) probe_one<HullLDS, G64>(m, G, patch, qs, i, out, lane == 0, H);
  } else if constexpr (PATH == P_LDS_G16) {
    HullLDS H{pool, nslots};
    hull_load<G64>(m, G, H);
    wave_sync();
    const int row = lane >> 4;
    for (int i0 = 4 * blockIdx.x; i0 < nq; i0 += 4 * nblk) {
      const int i = i0 + row;
      const bool in = i < nq;          // (a row past the end repeats the first query of its workgroup and writes nothing)
      probe_one<HullLDS, G16>(m, G, patch, qs, in ? i : i0, out, in && (lane & 15) == 0, H);
    }
  } else {
    // the cell's list loaded the way k_narrow's fast path loads it (tu_narrow.hip): entry l and l + 64 in lane l
    for (int i = blockIdx.x; i < nq; i += nblk) {
      const unsigned int* o = m->hl_off + cells[i];
      const int a = (int)o[0], cnt = (int)(o[1] - o[0]);
      if (cnt < 1 || cnt > HL_MAX) {                    // (a list the product does not use: NaN)
        if (lane == 0) for (int k = 0; k < (patch ? 3 * NCPP : 3); k++) out[(patch ? 3 * NCPP : 3) * i + k] = __int_as_float(0x7fc00000);
        continue;
      }
      const float* E = m->hl_entry + 4 * (size_t)a;
      HullSub S;
#pragma unroll
      for (int q = 0; q < 2; q++) {
        int k = lane + WAVE * q;
        bool inl = k < cnt;
        float4 ev; ev.x = 0.f; ev.y = 0.f; ev.z = 0.f; ev.w = 0.f;
        if (inl) ev = *(const float4*)(E + 4 * (size_t)k);
        S.x[q] = ev.x; S.y[q] = ev.y; S.z[q] = ev.z; S.i[q] = inl ? __float_as_int(ev.w) : 0x7fffffff;
      }
      probe_one<HullSub, G64>(m, G, patch, qs, i, out, lane == 0, S);
    }
  }
}

__global__ __launch_bounds__(64) void k_hl_cell(const float* dl, int nq, int nblk, int* out) {
  for (int i = blockIdx.x * WAVE + wave_lane(); i < nq; i += nblk * WAVE) out[i] = hl_cell(dl + 3 * i);
}

__global__ __launch_bounds__(64) void k_sbt_bound(const float* T, const float* dl, int nq, int nblk, float* out) {
  for (int i = blockIdx.x * WAVE + wave_lane(); i < nq; i += nblk * WAVE) out[i] = sbt_bound(T, dl + 3 * i);
}

DEV void unpack_geom(const float* w, GeomW& G) {
  G.type = (int)w[0]; G.vadr = 0; G.vnum = 0;
  for (int i = 0; i < 3; i++) { G.size[i] = w[1 + i]; G.p[i] = w[13 + i]; G.c[i] = w[16 + i]; }
  for (int i = 0; i < 9; i++) G.R[i] = w[4 + i];
}

// narrowphase of a flat face (plane / box, geom 1) against the hull (geom 2) on the three paths that must agree: the fused step's narrow_pair<NoCache>,
// k_narrow's fast path narrow_pair_cached<HullSub, G64, true, true> on the cell light_first_cell() picks (tu_narrow.hip, so101_pipeline.hpp
// publish_candidates) and k_narrow's row pass narrow_pair_cached<HullLDS, G16, true> (four pairs per workgroup).  Pair i: geom 1 at
// pg[PAIR_WORDS i], geom 2 (type, size ignored: the hull) at + GEOM_WORDS; the bounding radii are the model's geom_rbound[2 i], [2 i + 1].
// out: PAIR_OUT floats per pair: settled (1 / 0, -1: the path does not take the pair), contacts valid mask, normal, NCPP distances, NCPP positions.
enum { Q_FUSED = 0, Q_FAST = 1, Q_ROWS = 2 };
#define PAIR_WORDS (2 * GEOM_WORDS)
#define PAIR_OUT (5 + 4 * NCPP)

DEV void pair_geoms(const DevModel* m, const float* pg, int i, int vnum, GeomW& G1, GeomW& G2, float& rb1, float& rb2) {
  unpack_geom(pg + PAIR_WORDS * i, G1);
  unpack_geom(pg + PAIR_WORDS * i + GEOM_WORDS, G2);
  G2.type = G_MESH; G2.vnum = vnum;
  rb1 = m->geom_rbound[2 * i]; rb2 = m->geom_rbound[2 * i + 1];
}

DEV void pair_store(float* o, float settled, const PairContacts& pc) {
  o[0] = settled; o[1] = (float)pc.valid;
  for (int k = 0; k < 3; k++) o[2 + k] = pc.nrm[k];
  for (int q = 0; q < NCPP; q++) { o[5 + q] = pc.dist[q]; for (int k = 0; k < 3; k++) o[5 + NCPP + 3 * q + k] = pc.pos[q][k]; }
}

template <int MODE>
__global__ __launch_bounds__(64) void k_pair(const DevModel* m, int vnum, const float* pg, int nq, int nblk, float* out) {
  __shared__ __attribute__((aligned(16))) float pool[3 * HULL_LDS_MAX];
  const int lane = wave_lane();
  if constexpr (MODE == Q_FUSED) {
    for (int i = blockIdx.x; i < nq; i += nblk) {
      GeomW G1, G2; float rb1, rb2;
      pair_geoms(m, pg, i, vnum, G1, G2, rb1, rb2);
      PairContacts pc;
      narrow_pair<NoCache>(m, G1, G2, 2 * i, 2 * i + 1, pc);
      if (lane == 0) pair_store(out + PAIR_OUT * i, 1.f, pc);
    }
  } else if constexpr (MODE == Q_FAST) {
    for (int i = blockIdx.x; i < nq; i += nblk) {
      GeomW G1, G2; float rb1, rb2;
      pair_geoms(m, pg, i, vnum, G1, G2, rb1, rb2);
      PairContacts pc;
      pc.valid = 0u;
      for (int k = 0; k < 3; k++) pc.nrm[k] = 0.f;
      for (int q = 0; q < NCPP; q++) { pc.dist[q] = 0.f; for (int k = 0; k < 3; k++) pc.pos[q][k] = 0.f; }
      const int cell = light_first_cell(G1, G2);
      int a = 0, cnt = 0;
      if (cell >= 0) { a = (int)m->hl_off[cell]; cnt = (int)(m->hl_off[cell + 1] - m->hl_off[cell]); }
      if (cnt < 1 || cnt > HL_MAX) { if (lane == 0) pair_store(out + PAIR_OUT * i, -1.f, pc); continue; }
      const float* E = m->hl_entry + 4 * (size_t)a;
      HullSub S1, S2;
#pragma unroll
      for (int q = 0; q < 2; q++) {
        int k = lane + WAVE * q;
        bool in = k < cnt;
        float4 ev; ev.x = 0.f; ev.y = 0.f; ev.z = 0.f; ev.w = 0.f;
        if (in) ev = *(const float4*)(E + 4 * (size_t)k);
        S2.x[q] = ev.x; S2.y[q] = ev.y; S2.z[q] = ev.z; S2.i[q] = in ? __float_as_int(ev.w) : 0x7fffffff;
        S1.x[q] = 0.f; S1.y[q] = 0.f; S1.z[q] = 0.f; S1.i[q] = 0x7fffffff;
      }
      const bool settled = narrow_pair_cached<HullSub, G64, true, true>(m, G1, G2, rb1, rb2, S1, S2, pc);
      if (lane == 0) pair_store(out + PAIR_OUT * i, settled ? 1.f : 0.f, pc);
    }
  } else {
    HullLDS H2{pool, hull_lds_slots(G_MESH, vnum)};
    GeomW GH; probe_geom(vnum, GH);
    hull_load<G64>(m, GH, H2);
    wave_sync();
    const int row = lane >> 4;
    for (int i0 = 4 * blockIdx.x; i0 < nq; i0 += 4 * nblk) {
      const int i = i0 + row;
      const bool in = i < nq;          // (a row past the end repeats the first pair of its workgroup and writes nothing)
      GeomW G1, G2; float rb1, rb2;
      pair_geoms(m, pg, in ? i : i0, vnum, G1, G2, rb1, rb2);
      HullLDS H1{pool, 0};             // (geom 1 is a plane or a box: nothing staged, as in k_narrow)
      PairContacts pc;
      const bool settled = narrow_pair_cached<HullLDS, G16, true>(m, G1, G2, rb1, rb2, H1, H2, pc);
      if (in && (lane & 15) == 0) pair_store(out + PAIR_OUT * i, settled ? 1.f : 0.f, pc);
    }
  }
}

__global__ __launch_bounds__(64) void k_first_cell(const float* g1, const float* g2, int nq, int nblk, int* out) {
  for (int i = blockIdx.x * WAVE + wave_lane(); i < nq; i += nblk * WAVE) {
    GeomW A, B;
    unpack_geom(g1 + GEOM_WORDS * i, A); unpack_geom(g2 + GEOM_WORDS * i, B);
    out[i] = light_first_cell(A, B);
  }
}

struct Probe {
  DevModel hm{};
  DevModel* dm = nullptr;
  int n = 0;
  std::vector<float> sbt, hle;
  std::vector<unsigned int> hlo;
  std::vector<void*> owned;
};

template <class T>
bool put(Probe* p, const T* v, size_t count, const T** out) {
  void* d = nullptr;
  if (hipMalloc(&d, (count ? count : 1) * sizeof(T)) != hipSuccess) return false;
  p->owned.push_back(d);
  if (count && hipMemcpy(d, v, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return false;
  *out = (const T*)d;
  return true;
}

// device copy of a host array for the length of one call
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4) == hipSuccess && hipMemset(p, 0, bytes ? bytes : 4) == hipSuccess; }
  bool in(const void* h, size_t bytes) { return alloc(bytes) && (!bytes || hipMemcpy(p, h, bytes, hipMemcpyHostToDevice) == hipSuccess); }
  bool out(void* h, size_t bytes) const { return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess && hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost) == hipSuccess; }
};

int blocks_for(int units) {
#ifdef SO101_EMU
  (void)units;
  return 1;                  // (one block of 64 OS threads walks every query: thread start-up dominates the emulation)
#else
  return units < 1 ? 1 : (units < 2048 ? units : 2048);
#endif
}

// the GPU build takes finite inputs only (non-finite directions are a test of the emulated build)
bool inputs_ok(const float* v, size_t count) {
#ifdef SO101_EMU
  (void)v; (void)count;
  return true;
#else
  for (size_t k = 0; k < count; k++) if (!std::isfinite(v[k])) return false;
  return true;
#endif
}

}  // namespace

extern "C" {

void probe_destroy(void* h) {
  Probe* p = (Probe*)h;
  if (!p) return;
  for (void* d : p->owned) (void)hipFree(d);
  delete p;
}

// V: n vertices, xyz interleaved.  Builds the hull's tables with the product's builder (so101_tables.hpp) and uploads them.
void* probe_create(const float* V, int n) {
  if (!V || n < 1 || !inputs_ok(V, 3 * (size_t)n)) return nullptr;
  Probe* p = new Probe();
  p->n = n;
  p->sbt.resize(SBT_DIM);
  build_support_bounds(V, n, p->sbt.data());
  p->hlo.resize(HL_CELLS + 1);
  build_support_lists(V, n, p->hle, p->hlo.data());
  std::vector<float> x(n), y(n), z(n);
  for (int k = 0; k < n; k++) { x[k] = V[3 * k]; y[k] = V[3 * k + 1]; z[k] = V[3 * k + 2]; }
  DevModel& M = p->hm;
  M.ngeom = 1; M.nvert = n;
  M.mpr_iter = 50; M.mpr_tol = 1e-6f;                    // (the scenes' opt_mpr_iterations / opt_mpr_tolerance: narrow_pair's iterative query)
  bool ok = put(p, x.data(), x.size(), &M.vx) && put(p, y.data(), y.size(), &M.vy) && put(p, z.data(), z.size(), &M.vz) &&
            put(p, p->sbt.data(), p->sbt.size(), &M.hull_sbt) && put(p, p->hle.data(), p->hle.size(), &M.hl_entry) &&
            put(p, p->hlo.data(), p->hlo.size(), &M.hl_off);
  void* dm = nullptr;
  ok = ok && hipMalloc(&dm, sizeof(DevModel)) == hipSuccess;
  if (dm) p->owned.push_back(dm);
  ok = ok && hipMemcpy(dm, &M, sizeof(DevModel), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) { probe_destroy(p); return nullptr; }
  p->dm = (DevModel*)dm;
  return p;
}

int probe_entry_count(void* h) { return h ? (int)(((Probe*)h)->hle.size() / 4) : -1; }

// the host tables: sbt[SBT_DIM], off[HL_CELLS + 1], entries[4 * probe_entry_count()]
int probe_tables(void* h, float* sbt, unsigned int* off, float* entries) {
  Probe* p = (Probe*)h;
  if (!p) return -1;
  memcpy(sbt, p->sbt.data(), p->sbt.size() * sizeof(float));
  memcpy(off, p->hlo.data(), p->hlo.size() * sizeof(unsigned int));
  if (!p->hle.empty()) memcpy(entries, p->hle.data(), p->hle.size() * sizeof(float));
  return 0;
}

// nq support queries (patch = 0: directions, 3 floats each; patch = 1: frames f | u | v, 9 floats each) on one path; cells: the list cell of
// each query (path P_SUB only).  out: 3 or 3 NCPP floats per query.  0 = done, < 0 = rejected arguments or a HIP error.
int probe_support(void* h, int path, int nslots, int patch, const float* qs, const int* cells, int nq, float* out) {
  Probe* p = (Probe*)h;
  if (!p || path < 0 || path >= P_COUNT || nq < 0 || (patch != 0 && patch != 1)) return -1;
  if ((path == P_LDS || path == P_LDS_G16) && nslots != 0 && nslots != 256 && nslots != HULL_LDS_MAX) return -1;
  const size_t qw = patch ? 9 : 3, ow = patch ? 3 * NCPP : 3;
  if (nq == 0) return 0;
  if (!inputs_ok(qs, qw * nq)) return -2;
  if (path == P_SUB) for (int i = 0; i < nq; i++) if (!cells || cells[i] < 0 || cells[i] >= HL_CELLS) return -1;
  DevBuf dq, dc, dout;
  if (!dq.in(qs, qw * nq * sizeof(float)) || !dc.in(path == P_SUB ? (const void*)cells : nullptr, path == P_SUB ? nq * sizeof(int) : 0) ||
      !dout.alloc(ow * nq * sizeof(float)))
    return -3;
  const int nblk = blocks_for(path == P_LDS_G16 ? (nq + 3) / 4 : nq);
  const float* q = (const float*)dq.p; const int* c = (const int*)dc.p; float* o = (float*)dout.p;
  switch (path) {
    case P_NOCACHE: hipLaunchKernelGGL(k_support<P_NOCACHE>, dim3(nblk), dim3(64), 0, 0, p->dm, p->n, nslots, patch, q, c, nq, nblk, o); break;
    case P_HULLCACHE: hipLaunchKernelGGL(k_support<P_HULLCACHE>, dim3(nblk), dim3(64), 0, 0, p->dm, p->n, nslots, patch, q, c, nq, nblk, o); break;
    case P_LDS: hipLaunchKernelGGL(k_support<P_LDS>, dim3(nblk), dim3(64), 0, 0, p->dm, p->n, nslots, patch, q, c, nq, nblk, o); break;
    case P_LDS_G16: hipLaunchKernelGGL(k_support<P_LDS_G16>, dim3(nblk), dim3(64), 0, 0, p->dm, p->n, nslots, patch, q, c, nq, nblk, o); break;
    default: hipLaunchKernelGGL(k_support<P_SUB>, dim3(nblk), dim3(64), 0, 0, p->dm, p->n, nslots, patch, q, c, nq, nblk, o); break;
  }
  return dout.out(out, ow * nq * sizeof(float)) ? 0 : -3;
}

// hl_cell of nq directions (3 floats each)
int probe_hl_cell(const float* dl, int nq, int* out) {
  if (nq < 0) return -1;
  if (nq == 0) return 0;
  if (!inputs_ok(dl, 3 * (size_t)nq)) return -2;
  DevBuf dd, dout;
  if (!dd.in(dl, 3 * (size_t)nq * sizeof(float)) || !dout.alloc((size_t)nq * sizeof(int))) return -3;
  const int nblk = blocks_for((nq + WAVE - 1) / WAVE);
  hipLaunchKernelGGL(k_hl_cell, dim3(nblk), dim3(64), 0, 0, (const float*)dd.p, nq, nblk, (int*)dout.p);
  return dout.out(out, (size_t)nq * sizeof(int)) ? 0 : -3;
}

// sbt_bound of the hull's table at nq geom-frame directions.  The table is placed between two copies of SBT_DIM floats of `pad`: a result that
// depends on the pad value read outside the table.
int probe_sbt_bound(void* h, const float* dl, int nq, float pad, float* out) {
  Probe* p = (Probe*)h;
  if (!p || nq < 0) return -1;
  if (nq == 0) return 0;
  if (!inputs_ok(dl, 3 * (size_t)nq)) return -2;
  std::vector<float> T(3 * SBT_DIM, pad);
  memcpy(&T[SBT_DIM], p->sbt.data(), SBT_DIM * sizeof(float));
  DevBuf dt, dd, dout;
  if (!dt.in(T.data(), T.size() * sizeof(float)) || !dd.in(dl, 3 * (size_t)nq * sizeof(float)) || !dout.alloc((size_t)nq * sizeof(float))) return -3;
  const int nblk = blocks_for((nq + WAVE - 1) / WAVE);
  hipLaunchKernelGGL(k_sbt_bound, dim3(nblk), dim3(64), 0, 0, (const float*)dt.p + SBT_DIM, (const float*)dd.p, nq, nblk, (float*)dout.p);
  return dout.out(out, (size_t)nq * sizeof(float)) ? 0 : -3;
}

// the narrowphase of nq (flat face, hull) pairs on one path (Q_*): pg = PAIR_WORDS floats per pair, rb = 2 bounding radii per pair,
// out = PAIR_OUT floats per pair
int probe_pairs(void* h, int mode, const float* pg, const float* rb, int nq, float* out) {
  Probe* p = (Probe*)h;
  if (!p || mode < Q_FUSED || mode > Q_ROWS || nq < 0) return -1;
  if (nq == 0) return 0;
  if (!inputs_ok(pg, PAIR_WORDS * (size_t)nq) || !inputs_ok(rb, 2 * (size_t)nq)) return -2;
  for (int i = 0; i < nq; i++) { int t = (int)pg[PAIR_WORDS * i]; if (t != G_PLANE && t != G_BOX) return -1; }
  DevBuf dg, dr, dm, dout;
  if (!dg.in(pg, PAIR_WORDS * (size_t)nq * sizeof(float)) || !dr.in(rb, 2 * (size_t)nq * sizeof(float)) || !dout.alloc(PAIR_OUT * (size_t)nq * sizeof(float)))
    return -3;
  DevModel M = p->hm;                                    // (this call's bounding radii: geom_rbound[2 i], [2 i + 1])
  M.geom_rbound = (const float*)dr.p;
  if (!dm.in(&M, sizeof M)) return -3;
  const DevModel* m = (const DevModel*)dm.p;
  const float* g = (const float*)dg.p; float* o = (float*)dout.p;
  const int nblk = blocks_for(mode == Q_ROWS ? (nq + 3) / 4 : nq);
  if (mode == Q_FUSED) hipLaunchKernelGGL(k_pair<Q_FUSED>, dim3(nblk), dim3(64), 0, 0, m, p->n, g, nq, nblk, o);
  else if (mode == Q_FAST) hipLaunchKernelGGL(k_pair<Q_FAST>, dim3(nblk), dim3(64), 0, 0, m, p->n, g, nq, nblk, o);
  else hipLaunchKernelGGL(k_pair<Q_ROWS>, dim3(nblk), dim3(64), 0, 0, m, p->n, g, nq, nblk, o);
  return dout.out(out, PAIR_OUT * (size_t)nq * sizeof(float)) ? 0 : -3;
}

// light_first_cell of nq geom pairs, each geom packed in GEOM_WORDS floats
int probe_first_cell(const float* g1, const float* g2, int nq, int* out) {
  if (nq < 0) return -1;
  if (nq == 0) return 0;
  if (!inputs_ok(g1, GEOM_WORDS * (size_t)nq) || !inputs_ok(g2, GEOM_WORDS * (size_t)nq)) return -2;
  DevBuf d1, d2, dout;
  if (!d1.in(g1, GEOM_WORDS * (size_t)nq * sizeof(float)) || !d2.in(g2, GEOM_WORDS * (size_t)nq * sizeof(float)) || !dout.alloc((size_t)nq * sizeof(int))) return -3;
  const int nblk = blocks_for((nq + WAVE - 1) / WAVE);
  hipLaunchKernelGGL(k_first_cell, dim3(nblk), dim3(64), 0, 0, (const float*)d1.p, (const float*)d2.p, nq, nblk, (int*)dout.p);
  return dout.out(out, (size_t)nq * sizeof(int)) ? 0 : -3;
}

}  // extern "C"
