// TEST HARNESS ONLY - device probes of three layers that the solution-level comparisons cannot see, for tests/test_blocks_emu.py and
// tests/test_blocks_gpu.py (cases, references and checks: tests/blocks_cases.py):
//   A. the per-contact cone blocks and scalar rows of both Newton solvers (so101_newton.hpp contact_cost / contact_line / row_cost, so101_tree.hpp
//      contact_block / contact_line / scalar_block), one case per lane: no LDS, no cross-lane traffic;
//   B. the wave primitives of wave.hpp (under emulation: of tests/hostemu/wave_emu.hpp), one case per 64-lane workgroup;
//   C. the small math of so101_math.hpp, one case per lane.
// tests/devprims/blocks.py builds this file with hipcc for gfx950 (the product's flags) or with g++ against the lane-thread emulation, like
// support_probe.hip.  The product never links it.  No kernel here loops on the device or touches global memory beyond its case arrays (the
// mfma_32x32x2 calls of k_mfma are a compile-time count, unrolled).
#include <hip/hip_runtime.h>
#ifdef SO101_EMU
thread_local emu_idx threadIdx;
thread_local emu_idx blockIdx;
thread_local EmuBlock* emu_blk;
#endif
#include "../../so101_sim_amd/csrc/so101_device.hpp"
#include "../../so101_sim_amd/csrc/so101_tree.hpp"

#include <cmath>

#define SO100_CON_OUT 39      // want_h on: cost, force[6], Hc[21] (packed lower triangle), zone; want_h off: cost, force[6], zone; contact_line d1, d2
#define TREE_CON_OUT 52       // want_h on: cost, force[6], Hc[36]; want_h off: cost, force[6]; contact_line d1, d2
#define QUAT_IN 32            // qa[4], qb[4], s[6] (packed symmetric), R[9], m[9]
#define QUAT_OUT 36           // quat2mat(qa)[9], mulquat(qa, qb)[4], normquat(qa)[4], normalize3(qb[0..2])[3] + its return, rotsym(R, s)[6], mat2quat(m)[4], rotvecquat(qb[1..3], qa)[3], pad[2]
#define WAVE_CH 4             // float and int channels per lane of probe_wave, in and out

namespace {

// ---- one case per lane: a functor per probe; the GPU build runs lane i of a flat launch on case i, the emulated build a host loop (the functions
// under test are pure: nothing crosses lanes)
#ifdef SO101_EMU
template <class F, class... A>
void run_lanes(int n, A... a) { for (int i = 0; i < n; i++) F()(i, a...); }
#else
template <class F, class... A>
__global__ __launch_bounds__(256) void k_lanes(int n, A... a) {
  int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i < n) F()(i, a...);
}
template <class F, class... A>
void run_lanes(int n, A... a) { hipLaunchKernelGGL((k_lanes<F, A...>), dim3((n + 255) / 256), dim3(256), 0, 0, n, a...); }
#endif

struct So100Contact {
  DEV void operator()(int i, const int* dim, const float* mu, const float* fr, const float* D, const float* r, const float* dr, float* out) const {
    ConReg C;
    for (int c = 0; c < 12; c++) for (int j = 0; j < 6; j++) C.J[c][j] = 0.f;
    for (int j = 0; j < 6; j++) { C.Dj[j] = D[6 * i + j]; C.aref[j] = 0.f; }
    for (int j = 0; j < 5; j++) C.fr[j] = fr[5 * i + j];
    C.mu = mu[i]; C.dim = dim[i]; C.g0 = 0; C.g1 = -1;
    float rr[6], dd[6], f[6], Hc[21];
    for (int j = 0; j < 6; j++) { rr[j] = r[6 * i + j]; dd[j] = dr[6 * i + j]; }
    float* o = out + SO100_CON_OUT * (size_t)i;
    int zone = -1;
    for (int k = 0; k < 21; k++) Hc[k] = 3.f;          // (finite garbage: every zero that comes out is contact_cost's own)
    for (int j = 0; j < 6; j++) f[j] = 3.f;
    o[0] = contact_cost(C, rr, f, Hc, true, &zone);
    for (int j = 0; j < 6; j++) o[1 + j] = f[j];
    for (int k = 0; k < 21; k++) o[7 + k] = Hc[k];
    o[28] = (float)zone;
    zone = -1;
    for (int j = 0; j < 6; j++) f[j] = 3.f;
    o[29] = contact_cost(C, rr, f, Hc, false, &zone);
    for (int j = 0; j < 6; j++) o[30 + j] = f[j];
    o[36] = (float)zone;
    contact_line(C, rr, dd, &o[37], &o[38]);
  }
};

struct TreeContact {
  DEV void operator()(int i, const int* dim, const float* mu, const float* fr, const float* D, const float* r, const float* dr, float* out) const {
    tv32::TCon C;
    for (int j = 0; j < 3; j++) C.pos[j] = 0.f;
    for (int j = 0; j < 9; j++) C.frame[j] = 0.f;
    C.dist = 0.f; C.mu = mu[i];
    for (int j = 0; j < 5; j++) { C.fric[j] = fr[5 * i + j]; C.solimp[j] = 0.f; }
    C.solref[0] = 0.f; C.solref[1] = 0.f;
    C.g1 = 0; C.g2 = 0; C.b1 = 0; C.b2 = 0; C.dim = dim[i]; C.row = 0;
    float DD[6], rr[6], dd[6], f[6], Hc[36];
    for (int j = 0; j < 6; j++) { DD[j] = D[6 * i + j]; rr[j] = r[6 * i + j]; dd[j] = dr[6 * i + j]; }
    float* o = out + TREE_CON_OUT * (size_t)i;
    o[0] = tv32::tree::contact_block(C, DD, dim[i], rr, f, Hc, true);
    for (int j = 0; j < 6; j++) o[1 + j] = f[j];
    for (int k = 0; k < 36; k++) o[7 + k] = Hc[k];
    o[43] = tv32::tree::contact_block(C, DD, dim[i], rr, f, Hc, false);
    for (int j = 0; j < 6; j++) o[44 + j] = f[j];
    tv32::tree::contact_line(C, DD, dim[i], rr, dd, &o[50], &o[51]);
  }
};

struct So100Row {        // out: cost, force, h
  DEV void operator()(int i, const float* R, const float* floss, const float* jar, float* out) const {
    Row1 w; w.dof = 0; w.sign = 1.f; w.R = R[i]; w.aref = 0.f; w.f = 0.f; w.floss = floss[i]; w.Ainv = 0.f; w.pad = 0.f;
    out[3 * i] = row_cost(w, jar[i], &out[3 * i + 1], &out[3 * i + 2]);
  }
};

struct TreeScalar {      // out: cost, force, h
  DEV void operator()(int i, const int* type, const float* D, const float* R, const float* fl, const float* r, float* out) const {
    out[3 * i] = tv32::tree::scalar_block(type[i], D[i], R[i], fl[i], r[i], &out[3 * i + 1], &out[3 * i + 2]);
  }
};

struct SinCos {
  DEV void operator()(int i, const float* x, float* s, float* c) const { sincos_f(x[i], &s[i], &c[i]); }
};

struct Quat {
  DEV void operator()(int i, const float* in, float* out) const {
    const float* a = in + QUAT_IN * (size_t)i;
    float* o = out + QUAT_OUT * (size_t)i;
    float q[4], v[3];
    quat2mat(o, a);
    mulquat(o + 9, a, a + 4);
    for (int k = 0; k < 4; k++) q[k] = a[k];
    normquat(q);
    for (int k = 0; k < 4; k++) o[13 + k] = q[k];
    for (int k = 0; k < 3; k++) v[k] = a[4 + k];
    o[20] = normalize3(v);
    for (int k = 0; k < 3; k++) o[17 + k] = v[k];
    rotsym(o + 21, a + 14, a + 8);
    mat2quat(o + 27, a + 23);
    rotvecquat(o + 31, a + 5, a);
    o[34] = 0.f; o[35] = 0.f;
  }
};

struct Imp {
  DEV void operator()(int i, const float* solimp, const float* pos, float* out) const { out[i] = impedance(solimp + 5 * (size_t)i, pos[i]); }
};

struct Rng {
  DEV void operator()(int i, const unsigned long long* seed, const unsigned long long* env, const unsigned int* ep, const unsigned int* draw, float* out) const {
    out[i] = rng_uniform(seed[i], env[i], ep[i], draw[i]);
  }
};

struct Tri {
  DEV void operator()(int i, int n, int* out) const { out[i] = tri(i / n, i % n); }
};

// ---- wave primitives: workgroup = case, lane l reads fin / iin [case][channel][l] and writes fout / iout the same way
enum { W_MAX = 0, W_MIN_I, W_SUM, W_SUM_ROWS, W_SUM_ROW0, W_BALLOT, W_ARGMAX, W_ARGMAX3, W_ROW_ARGMAX3, W_ROW_ARGMAX, W_GET, W_BCAST, W_XOR32, W_COUNT };

template <int OP>
__global__ __launch_bounds__(64) void k_wave(const float* fin, const int* iin, float* fout, int* iout) {
  const int lane = wave_lane();
  const size_t base = (size_t)blockIdx.x * WAVE_CH * WAVE;
  float f[WAVE_CH]; int n[WAVE_CH];
#pragma unroll
  for (int c = 0; c < WAVE_CH; c++) { f[c] = fin[base + WAVE * c + lane]; n[c] = iin[base + WAVE * c + lane]; }
  float of[WAVE_CH] = {0.f, 0.f, 0.f, 0.f}; int on[WAVE_CH] = {0, 0, 0, 0};
  if constexpr (OP == W_MAX) of[0] = wave_max_f(f[0]);
  else if constexpr (OP == W_MIN_I) on[0] = wave_min_i(n[0]);
  else if constexpr (OP == W_SUM) of[0] = wave_sum_f(f[0]);
  else if constexpr (OP == W_SUM_ROWS) of[0] = wave_sum_rows_f(f[0], false);
  else if constexpr (OP == W_SUM_ROW0) of[0] = wave_sum_rows_f(f[0], true);
  else if constexpr (OP == W_BALLOT) {
    unsigned long long m = wave_ballot(n[0] != 0);
    on[0] = wave_prefix(m); on[1] = (int)(unsigned int)m; on[2] = (int)(unsigned int)(m >> 32);
  } else if constexpr (OP == W_ARGMAX) {
    of[0] = f[0]; on[0] = n[0];
    wave_argmax(of[0], on[0]);
  } else if constexpr (OP == W_ARGMAX3) {
    of[0] = f[0]; on[0] = n[0]; of[1] = f[1]; of[2] = f[2]; of[3] = f[3];
    wave_argmax3(of[0], on[0], of[1], of[2], of[3]);
  } else if constexpr (OP == W_ROW_ARGMAX3) {
    // int channel 1: 1 in every lane of an active row, 0 in every lane of a row that is branched out (the contract of wave.hpp)
    if (n[1] != 0) {
      of[0] = f[0]; on[0] = n[0]; of[1] = f[1]; of[2] = f[2]; of[3] = f[3];
      row_argmax3(of[0], on[0], of[1], of[2], of[3]);
    }
  } else if constexpr (OP == W_ROW_ARGMAX) {
    if (n[1] != 0) {
      of[0] = f[0]; on[0] = n[0];
      row_argmax(of[0], on[0]);
    }
  } else if constexpr (OP == W_GET) {
    // int channel 1 of lane 0: the source lane, wave-uniform
    const int src = wave_uniform_i(iin[base + WAVE]) & 63;
    of[0] = wave_get_f(f[0], src); on[0] = wave_get_i(n[0], src);
  } else if constexpr (OP == W_BCAST) {
    // int channel 1: each lane's own source lane
    of[0] = wave_bcast_f(f[0], n[1] & 63); on[0] = wave_bcast_i(n[0], n[1] & 63);
  } else if constexpr (OP == W_XOR32) of[0] = wave_xor32_f(f[0]);
#pragma unroll
  for (int c = 0; c < WAVE_CH; c++) { fout[base + WAVE * c + lane] = of[c]; iout[base + WAVE * c + lane] = on[c]; }
}

// D (32 x 32) = sum over NCALL of A_c (32 x 2) B_c (2 x 32): a, b [case][call][lane], out [case][lane][16]
template <int NCALL>
__global__ __launch_bounds__(64) void k_mfma(const float* a, const float* b, float* out) {
  const int lane = wave_lane();
  mfma_acc16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
#pragma unroll
  for (int c = 0; c < NCALL; c++) {
    const size_t at = ((size_t)blockIdx.x * NCALL + c) * WAVE + lane;
    acc = mfma_32x32x2(a[at], b[at], acc);
  }
#pragma unroll
  for (int r = 0; r < 16; r++) out[((size_t)blockIdx.x * WAVE + lane) * 16 + r] = acc[r];
}

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4) == hipSuccess && hipMemset(p, 0, bytes ? bytes : 4) == hipSuccess; }
  bool in(const void* h, size_t bytes) { return alloc(bytes) && (!bytes || hipMemcpy(p, h, bytes, hipMemcpyHostToDevice) == hipSuccess); }
  bool out(void* h, size_t bytes) const { return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess && hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost) == hipSuccess; }
};

// the GPU build takes finite inputs only
bool inputs_ok(const float* v, size_t count) {
#ifdef SO101_EMU
  (void)v; (void)count;
  return true;
#else
  for (size_t k = 0; k < count; k++) if (!std::isfinite(v[k])) return false;
  return true;
#endif
}

template <class F>
int run_contacts(int n, int min_dim, const int* dim, const float* mu, const float* fr, const float* D, const float* r, const float* dr, int ow, float* out) {
  if (n < 1 || n > 4096) return -1;
  for (int i = 0; i < n; i++) if (dim[i] < min_dim || dim[i] > 6 || dim[i] == 2 || dim[i] == 5) return -1;
  const size_t N = (size_t)n;
  if (!inputs_ok(mu, N) || !inputs_ok(fr, 5 * N) || !inputs_ok(D, 6 * N) || !inputs_ok(r, 6 * N) || !inputs_ok(dr, 6 * N)) return -2;
  DevBuf bd, bm, bf, bD, br, bdr, bo;
  if (!bd.in(dim, N * sizeof(int)) || !bm.in(mu, N * sizeof(float)) || !bf.in(fr, 5 * N * sizeof(float)) || !bD.in(D, 6 * N * sizeof(float)) ||
      !br.in(r, 6 * N * sizeof(float)) || !bdr.in(dr, 6 * N * sizeof(float)) || !bo.alloc(ow * N * sizeof(float)))
    return -3;
  run_lanes<F>(n, (const int*)bd.p, (const float*)bm.p, (const float*)bf.p, (const float*)bD.p, (const float*)br.p, (const float*)bdr.p, (float*)bo.p);
  return bo.out(out, ow * N * sizeof(float)) ? 0 : -3;
}

template <int OP>
void launch_wave(int ncase, const float* fin, const int* iin, float* fout, int* iout) {
  hipLaunchKernelGGL(k_wave<OP>, dim3(ncase), dim3(64), 0, 0, fin, iin, fout, iout);
}

}  // namespace

extern "C" {

// n <= 4096 contacts, one per lane: dim[n] (0 = dropped, 1, 3, 4, 6), mu[n], fr[n][5] (friction of rows 1 .. 5), D[n][6], r[n][6], dr[n][6];
// out[n][SO100_CON_OUT]
int probe_so100_contact(int n, const int* dim, const float* mu, const float* fr, const float* D, const float* r, const float* dr, float* out) {
  return run_contacts<So100Contact>(n, 0, dim, mu, fr, D, r, dr, SO100_CON_OUT, out);
}
// the same inputs (dim >= 1) through the tree engine's blocks; out[n][TREE_CON_OUT]
int probe_tree_contact(int n, const int* dim, const float* mu, const float* fr, const float* D, const float* r, const float* dr, float* out) {
  return run_contacts<TreeContact>(n, 1, dim, mu, fr, D, r, dr, TREE_CON_OUT, out);
}

int probe_so100_row(int n, const float* R, const float* floss, const float* jar, float* out) {
  if (n < 1 || n > 4096) return -1;
  const size_t N = (size_t)n;
  if (!inputs_ok(R, N) || !inputs_ok(floss, N) || !inputs_ok(jar, N)) return -2;
  DevBuf bR, bf, bj, bo;
  if (!bR.in(R, N * 4) || !bf.in(floss, N * 4) || !bj.in(jar, N * 4) || !bo.alloc(3 * N * 4)) return -3;
  run_lanes<So100Row>(n, (const float*)bR.p, (const float*)bf.p, (const float*)bj.p, (float*)bo.p);
  return bo.out(out, 3 * N * 4) ? 0 : -3;
}

// type: TR_FRICTION 0, TR_LIMIT 1, TR_EQUALITY 3
int probe_tree_scalar(int n, const int* type, const float* D, const float* R, const float* fl, const float* r, float* out) {
  if (n < 1 || n > 4096) return -1;
  const size_t N = (size_t)n;
  if (!inputs_ok(D, N) || !inputs_ok(R, N) || !inputs_ok(fl, N) || !inputs_ok(r, N)) return -2;
  DevBuf bt, bD, bR, bf, br, bo;
  if (!bt.in(type, N * 4) || !bD.in(D, N * 4) || !bR.in(R, N * 4) || !bf.in(fl, N * 4) || !br.in(r, N * 4) || !bo.alloc(3 * N * 4)) return -3;
  run_lanes<TreeScalar>(n, (const int*)bt.p, (const float*)bD.p, (const float*)bR.p, (const float*)bf.p, (const float*)br.p, (float*)bo.p);
  return bo.out(out, 3 * N * 4) ? 0 : -3;
}

int probe_sincos(int n, const float* x, float* s, float* c) {
  if (n < 1 || n > (1 << 20)) return -1;
  const size_t N = (size_t)n;
  if (!inputs_ok(x, N)) return -2;
  DevBuf bx, bs, bc;
  if (!bx.in(x, N * 4) || !bs.alloc(N * 4) || !bc.alloc(N * 4)) return -3;
  run_lanes<SinCos>(n, (const float*)bx.p, (float*)bs.p, (float*)bc.p);
  return bs.out(s, N * 4) && bc.out(c, N * 4) ? 0 : -3;
}

// in[n][QUAT_IN], out[n][QUAT_OUT]
int probe_quat(int n, const float* in, float* out) {
  if (n < 1 || n > 65536) return -1;
  const size_t N = (size_t)n;
  if (!inputs_ok(in, QUAT_IN * N)) return -2;
  DevBuf bi, bo;
  if (!bi.in(in, QUAT_IN * N * 4) || !bo.alloc(QUAT_OUT * N * 4)) return -3;
  run_lanes<Quat>(n, (const float*)bi.p, (float*)bo.p);
  return bo.out(out, QUAT_OUT * N * 4) ? 0 : -3;
}

int probe_impedance(int n, const float* solimp, const float* pos, float* out) {
  if (n < 1 || n > 65536) return -1;
  const size_t N = (size_t)n;
  if (!inputs_ok(solimp, 5 * N) || !inputs_ok(pos, N)) return -2;
  DevBuf bs, bp, bo;
  if (!bs.in(solimp, 5 * N * 4) || !bp.in(pos, N * 4) || !bo.alloc(N * 4)) return -3;
  run_lanes<Imp>(n, (const float*)bs.p, (const float*)bp.p, (float*)bo.p);
  return bo.out(out, N * 4) ? 0 : -3;
}

int probe_rng(int n, const unsigned long long* seed, const unsigned long long* env, const unsigned int* ep, const unsigned int* draw, float* out) {
  if (n < 1 || n > 65536) return -1;
  const size_t N = (size_t)n;
  DevBuf bs, be, bp, bd, bo;
  if (!bs.in(seed, N * 8) || !be.in(env, N * 8) || !bp.in(ep, N * 4) || !bd.in(draw, N * 4) || !bo.alloc(N * 4)) return -3;
  run_lanes<Rng>(n, (const unsigned long long*)bs.p, (const unsigned long long*)be.p, (const unsigned int*)bp.p, (const unsigned int*)bd.p, (float*)bo.p);
  return bo.out(out, N * 4) ? 0 : -3;
}

// out[n * n]: tri(i, j) at i * n + j
int probe_tri(int n, int* out) {
  if (n < 1 || n > 64) return -1;
  DevBuf bo;
  if (!bo.alloc((size_t)n * n * 4)) return -3;
  run_lanes<Tri>(n * n, n, (int*)bo.p);
  return bo.out(out, (size_t)n * n * 4) ? 0 : -3;
}

// op: the W_ enumeration; fin / iin / fout / iout [ncase][WAVE_CH][64]
int probe_wave(int op, int ncase, const float* fin, const int* iin, float* fout, int* iout) {
  if (op < 0 || op >= W_COUNT || ncase < 1 || ncase > 4096) return -1;
  const size_t W = (size_t)ncase * WAVE_CH * WAVE;
  if (!inputs_ok(fin, W)) return -2;
  DevBuf bf, bi, of, oi;
  if (!bf.in(fin, W * 4) || !bi.in(iin, W * 4) || !of.alloc(W * 4) || !oi.alloc(W * 4)) return -3;
  const float* f = (const float*)bf.p; const int* i = (const int*)bi.p; float* a = (float*)of.p; int* b = (int*)oi.p;
  switch (op) {
    case W_MAX: launch_wave<W_MAX>(ncase, f, i, a, b); break;
    case W_MIN_I: launch_wave<W_MIN_I>(ncase, f, i, a, b); break;
    case W_SUM: launch_wave<W_SUM>(ncase, f, i, a, b); break;
    case W_SUM_ROWS: launch_wave<W_SUM_ROWS>(ncase, f, i, a, b); break;
    case W_SUM_ROW0: launch_wave<W_SUM_ROW0>(ncase, f, i, a, b); break;
    case W_BALLOT: launch_wave<W_BALLOT>(ncase, f, i, a, b); break;
    case W_ARGMAX: launch_wave<W_ARGMAX>(ncase, f, i, a, b); break;
    case W_ARGMAX3: launch_wave<W_ARGMAX3>(ncase, f, i, a, b); break;
    case W_ROW_ARGMAX3: launch_wave<W_ROW_ARGMAX3>(ncase, f, i, a, b); break;
    case W_ROW_ARGMAX: launch_wave<W_ROW_ARGMAX>(ncase, f, i, a, b); break;
    case W_GET: launch_wave<W_GET>(ncase, f, i, a, b); break;
    case W_BCAST: launch_wave<W_BCAST>(ncase, f, i, a, b); break;
    default: launch_wave<W_XOR32>(ncase, f, i, a, b); break;
  }
  return of.out(fout, W * 4) && oi.out(iout, W * 4) ? 0 : -3;
}

// a, b [ncase][ncall][64], ncall 1, 3 or 18 (the Hessian's count); out [ncase][64][16]
int probe_mfma(int ncase, int ncall, const float* a, const float* b, float* out) {
  if (ncase < 1 || ncase > 4096 || (ncall != 1 && ncall != 3 && ncall != 18)) return -1;
  const size_t W = (size_t)ncase * ncall * WAVE, O = (size_t)ncase * WAVE * 16;
  if (!inputs_ok(a, W) || !inputs_ok(b, W)) return -2;
  DevBuf ba, bb, bo;
  if (!ba.in(a, W * 4) || !bb.in(b, W * 4) || !bo.alloc(O * 4)) return -3;
  const float* pa = (const float*)ba.p; const float* pb = (const float*)bb.p; float* po = (float*)bo.p;
  if (ncall == 1) hipLaunchKernelGGL(k_mfma<1>, dim3(ncase), dim3(64), 0, 0, pa, pb, po);
  else if (ncall == 3) hipLaunchKernelGGL(k_mfma<3>, dim3(ncase), dim3(64), 0, 0, pa, pb, po);
  else hipLaunchKernelGGL(k_mfma<18>, dim3(ncase), dim3(64), 0, 0, pa, pb, po);
  return bo.out(out, O * 4) ? 0 : -3;
}

}  // extern "C"
