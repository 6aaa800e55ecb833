// TEST HARNESS ONLY - device probe of the two broadphases, for tests/test_broadphase_emu.py and tests/test_broadphase_gpu.py (reference, cases and
// checks: tests/broadphase_ref.py, tests/broadphase_cases.py).  tests/devprims/broadphase.py builds this file three times, with hipcc for
// gfx950 (the product's flags) or with g++ against the lane-thread emulation of tests/hostemu, like support_probe.hip:
//   -DBP_ENGINE=0    so101_device.hpp broadphase() + obb_filter() on EnvLDS      (SO100: NDYN dynamic bodies, MAXGEOM geoms, MAXCAND candidates)
//   -DBP_ENGINE=32   so101_tree.hpp broadphase() on TreeLDS, TREE_VARIANT 32      (ALOHA: TB bodies, 128 geoms, TCAND 256)
//   -DBP_ENGINE=64   the same with TREE_VARIANT 64, selected as tu_tree64.hip does (Dining: 256 geoms, TCAND 512)
// The product never links it.  A handle holds the geometry part of a DevModel built from a scene blob by the product's own check_geometry() /
// upload_geometry() (so101_host.hpp; SO101_NO_SBT in the environment leaves the support-bound tables out, as in the product).  A query is one
// set of body frames; one 64-lane workgroup per query writes them into its __shared__ EnvLDS / TreeLDS, calls the product's broadphase()
// unchanged and copies out the candidate count, the whole candidate store and the overflow bit.  The store is filled with 0xffffffff before the
// call and copied out raw, so a count beyond what was written, or a write beyond the store's use, shows in the test.  On the GPU it is one
// workgroup per query; the emulated build runs one workgroup, which walks the queries.  Beyond the product's own loops the kernels loop over the
// copy in and out; they touch no global memory beyond the model and the case arrays.  The GPU build takes finite frames only.
#include <hip/hip_runtime.h>
#ifdef SO101_EMU
thread_local emu_idx threadIdx;
thread_local emu_idx blockIdx;
thread_local EmuBlock* emu_blk;
#endif
#ifndef BP_ENGINE
#define BP_ENGINE 0
#endif
#include "../../so101_sim_amd/csrc/so101_host.hpp"
#if BP_ENGINE == 0
#include "../../so101_sim_amd/csrc/so101_device.hpp"
#define BP_NB NDYN
#define BP_CAP MAXCAND
#define BP_NGEOM MAXGEOM
#else
#if BP_ENGINE == 64
#define TREE_VARIANT 64
#endif
#include "../../so101_sim_amd/csrc/so101_tree.hpp"
using namespace TREE_NS;
#define BP_NB TB
#define BP_CAP TCAND
#define BP_NGEOM TGEOM
#endif

#include <cmath>
#include <string>
#include <vector>

namespace {

// the queries of one workgroup: its own on the GPU, all of them under emulation (thread start-up dominates there)
#ifdef SO101_EMU
#define BP_QUERIES(q) for (int q = 0; q < nq; q++)
#else
#define BP_QUERIES(q) const int q = (int)blockIdx.x; if (q < nq)
#endif

#if BP_ENGINE == 0
__global__ __launch_bounds__(64) void k_broadphase(const DevModel* m, const float* xpos, const float* xmat, int nq, int* ncand, unsigned int* cand, int* over) {
  __shared__ EnvLDS L;
  const int lane = wave_lane();
  BP_QUERIES(q) {
    wave_sync();
    for (int i = lane; i < 3 * BP_NB; i += WAVE) (&L.xpos[0][0])[i] = xpos[(size_t)q * 3 * BP_NB + i];
    for (int i = lane; i < 9 * BP_NB; i += WAVE) (&L.xmat[0][0])[i] = xmat[(size_t)q * 9 * BP_NB + i];
    for (int k = lane; k < BP_CAP; k += WAVE) { L.cand[k][0] = 0xffffu; L.cand[k][1] = 0xffffu; }
    if (lane == 0) L.overflow = 0;
    wave_sync();
    broadphase(m, L);
    wave_sync();
    for (int k = lane; k < BP_CAP; k += WAVE) cand[(size_t)q * BP_CAP + k] = (unsigned int)L.cand[k][0] | ((unsigned int)L.cand[k][1] << 16);
    if (lane == 0) { ncand[q] = L.ncand; over[q] = L.overflow & 1; }
  }
}
#else
__global__ __launch_bounds__(64) void k_broadphase(const TreeModel* tm, const DevModel* m, const float* xpos, const float* xmat, int nq, int* ncand, unsigned int* cand,
                                                   int* over) {
  __shared__ TreeLDS L;
  const int lane = wave_lane();
  BP_QUERIES(q) {
    wave_sync();
    for (int i = lane; i < 3 * BP_NB; i += WAVE) (&L.xpos[0][0])[i] = xpos[(size_t)q * 3 * BP_NB + i];
    for (int i = lane; i < 9 * BP_NB; i += WAVE) (&L.xmat[0][0])[i] = xmat[(size_t)q * 9 * BP_NB + i];
    for (int k = lane; k < BP_CAP; k += WAVE) L.cand[k] = 0xffffffffu;
    if (lane == 0) L.flags = 0;
    wave_sync();
    const int n = tree::broadphase(tm, m, L);
    wave_sync();
    for (int k = lane; k < BP_CAP; k += WAVE) cand[(size_t)q * BP_CAP + k] = L.cand[k];
    if (lane == 0) { ncand[q] = L.ncand; over[q] = (L.flags & 1) | (n != L.ncand ? 2 : 0); }      // (bit 1: the returned count is not the stored one)
  }
}
#endif

struct Probe : HostHandle {
  DevModel hm{};
  DevModel* dm = nullptr;
#if BP_ENGINE != 0
  TreeModel tm{};
  TreeModel* dtm = nullptr;
#endif
};

thread_local std::string g_err;

// device copy of a host array for the length of one call
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4) == hipSuccess && hipMemset(p, 0xff, bytes ? bytes : 4) == hipSuccess; }
  bool in(const void* h, size_t bytes) { return alloc(bytes) && (!bytes || hipMemcpy(p, h, bytes, hipMemcpyHostToDevice) == hipSuccess); }
  bool out(void* h, size_t bytes) const { return hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost) == hipSuccess; }
};

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

const char* probe_error() { return g_err.c_str(); }

// bodies per query, candidate capacity, geom ceiling of this build
void probe_dims(int* out) { out[0] = BP_NB; out[1] = BP_CAP; out[2] = BP_NGEOM; out[3] = BP_ENGINE; }

void probe_destroy(void* h) {
  Probe* p = (Probe*)h;
  if (!p) return;
  (void)hipDeviceSynchronize();
  free_owned(p);
  delete p;
}

// The geometry of a scene blob (f32).  BP_ENGINE 0: geom_dyn [ngeom] (-1 or 0 .. NDYN - 1), geom_pos [ngeom][3] and geom_mat [ngeom][9] come
// from the caller, derived as build_model() of so101_hip.hip derives them (static geoms resolved to the world).  Tree builds: they are the blob's
// geom_body / geom_pos / quat2mat(geom_quat), as in tree_build() of so101_tree_host.hpp, and the three arguments are ignored.
void* probe_create(const void* blob, size_t bytes, const int* geom_dyn, const float* geom_pos, const float* geom_mat) {
  BlobView b;
  if (!blob || !b.parse(blob, bytes, g_err)) return nullptr;
  for (const char* n : {"nbody", "ngeom", "npair", "nvert"}) if (b.count(n) < 1) { g_err = std::string("blob entry missing: ") + n; return nullptr; }
  const int nbody = b.I("nbody")[0];
  if (nbody < 1 || nbody > 4096) { g_err = "nbody out of range"; return nullptr; }
  if (!check_geometry(b, (size_t)nbody, BP_NGEOM, g_err)) return nullptr;
  const int ng = b.I("ngeom")[0];
  Probe* p = new Probe();
  std::vector<int> gdyn;
  std::vector<float> gp, gm;
#if BP_ENGINE == 0
  if (!geom_dyn || !geom_pos || !geom_mat) { g_err = "the SO100 build needs geom_dyn, geom_pos and geom_mat"; delete p; return nullptr; }
  gdyn.assign(geom_dyn, geom_dyn + ng); gp.assign(geom_pos, geom_pos + 3 * (size_t)ng); gm.assign(geom_mat, geom_mat + 9 * (size_t)ng);
  for (int d : gdyn) if (d < -1 || d >= NDYN) { g_err = "geom_dyn out of range"; delete p; return nullptr; }
  if (!inputs_ok(gp.data(), gp.size()) || !inputs_ok(gm.data(), gm.size())) { g_err = "non-finite geom frames"; delete p; return nullptr; }
  const bool lists = true;
#else
  (void)geom_dyn; (void)geom_pos; (void)geom_mat;
  if (nbody > TB) { g_err = "too many bodies for this build"; delete p; return nullptr; }
  gdyn = b.I("geom_body"); gp = b.F("geom_pos");
  auto gquat = b.F("geom_quat");
  gm.resize(9 * (size_t)ng);
  for (int g = 0; g < ng; g++) h_quat2mat(&gm[9 * (size_t)g], &gquat[4 * (size_t)g]);
  const bool lists = false;
#endif
  bool ok = upload_geometry(p, b, gdyn, gp, gm, lists, p->hm) && upload_one(p, p->hm, &p->dm);
#if BP_ENGINE != 0
  p->tm.nbody = nbody; p->tm.ngeom = p->hm.ngeom; p->tm.npair = p->hm.npair;
  ok = ok && upload(p, b.I("geom_body"), &p->tm.geom_body) && upload_one(p, p->tm, &p->dtm);
#endif
  if (!ok) { g_err = p->err; probe_destroy(p); return nullptr; }
  return p;
}

// ngeom, npair, 1 when the support-bound tables are there
int probe_info(void* h, int* out) {
  Probe* p = (Probe*)h;
  if (!p) return -1;
  out[0] = p->hm.ngeom; out[1] = p->hm.npair; out[2] = p->hm.hull_sbt ? 1 : 0;
  return 0;
}

// what the product built: the packed pair words [npair] and the support-bound tables [ngeom][SBT_DIM] (zeros without them)
int probe_tables(void* h, unsigned int* packed, float* sbt) {
  Probe* p = (Probe*)h;
  if (!p) return -1;
  if (p->hm.npair && hipMemcpy(packed, p->hm.pair_packed, sizeof(unsigned int) * (size_t)p->hm.npair, hipMemcpyDeviceToHost) != hipSuccess) return -3;
  const size_t n = (size_t)p->hm.ngeom * SBT_DIM;
  if (!p->hm.hull_sbt) { for (size_t k = 0; k < n; k++) sbt[k] = 0.f; return 0; }
  return hipMemcpy(sbt, p->hm.hull_sbt, sizeof(float) * n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}

// the geoms' frames as the device holds them: geom_dyn [ngeom], geom_pos [ngeom][3], geom_mat [ngeom][9]
int probe_frames(void* h, int* gdyn, float* gpos, float* gmat) {
  Probe* p = (Probe*)h;
  if (!p) return -1;
  const size_t n = (size_t)p->hm.ngeom;
  return hipMemcpy(gdyn, p->hm.geom_dyn, sizeof(int) * n, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(gpos, p->hm.geom_pos, sizeof(float) * 3 * n, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(gmat, p->hm.geom_mat, sizeof(float) * 9 * n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}

// nq queries: xpos [nq][BP_NB][3], xmat [nq][BP_NB][9] (row-major rotations; the tree builds read body 0 = the world like any other body).
// out: ncand [nq], cand [nq][BP_CAP] (the whole store, geom1 | geom2 << 16; 0xffffffff where the call wrote nothing), over [nq].  0 = done, < 0 = rejected arguments or a HIP error.
int probe_broadphase(void* h, const float* xpos, const float* xmat, int nq, int* ncand, unsigned int* cand, int* over) {
  Probe* p = (Probe*)h;
  if (!p || nq < 0 || nq > (1 << 16)) return -1;
  if (nq == 0) return 0;
  if (!inputs_ok(xpos, 3 * (size_t)BP_NB * nq) || !inputs_ok(xmat, 9 * (size_t)BP_NB * nq)) return -2;
  DevBuf dp, dx, dn, dc, dv;
  if (!dp.in(xpos, sizeof(float) * 3 * BP_NB * (size_t)nq) || !dx.in(xmat, sizeof(float) * 9 * BP_NB * (size_t)nq) || !dn.alloc(sizeof(int) * (size_t)nq) ||
      !dc.alloc(sizeof(unsigned int) * BP_CAP * (size_t)nq) || !dv.alloc(sizeof(int) * (size_t)nq))
    return -3;
#ifdef SO101_EMU
  const int nblk = 1;
#else
  const int nblk = nq;
#endif
#if BP_ENGINE == 0
  hipLaunchKernelGGL(k_broadphase, dim3(nblk), dim3(64), 0, 0, (const DevModel*)p->dm, (const float*)dp.p, (const float*)dx.p, nq, (int*)dn.p, (unsigned int*)dc.p, (int*)dv.p);
#else
  hipLaunchKernelGGL(k_broadphase, dim3(nblk), dim3(64), 0, 0, (const TreeModel*)p->dtm, (const DevModel*)p->dm, (const float*)dp.p, (const float*)dx.p, nq, (int*)dn.p,
                     (unsigned int*)dc.p, (int*)dv.p);
#endif
  if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return -3;
  return dn.out(ncand, sizeof(int) * (size_t)nq) && dc.out(cand, sizeof(unsigned int) * BP_CAP * (size_t)nq) && dv.out(over, sizeof(int) * (size_t)nq) ? 0 : -3;
}

}  // extern "C"
