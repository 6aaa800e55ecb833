// Device helpers that belong to no engine: 3-vector / quaternion / symmetric-matrix arithmetic, the solimp impedance, the
// box-overlap tests of the overlap reward and the counter RNG.  Nothing here knows an engine's state or dimensions; the
// shared collision geometry (so101_geom.hpp) and both engines (so101_device.hpp, so101_tree.hpp) build on it.
#pragma once
#include <hip/hip_runtime.h>

#define DEV __device__ __forceinline__
// Stage clocks (100 MHz s_memrealtime ticks) for scripts/gpu_*.py: compiled in only with -DSO101_DEBUG_CLOCKS
// (python -m so101_sim_amd.build --clocks).  Production builds read the clock twice per solve (the scheduling hint
// of k_order) and nowhere else.
#ifdef SO101_DEBUG_CLOCKS
#define SO101_CLOCKS_ON 1
#define SO101_CLOCK() wall_clock64()
#else
#define SO101_CLOCKS_ON 0
#define SO101_CLOCK() 0ull
#endif
#ifndef SO101_COLLINEAR_REL
#define SO101_COLLINEAR_REL 1e-3f      // mpr_penetration: relative bound of the "origin on the v0-v1 segment" test, sin(angle) (kernel experiments: -DSO101_COLLINEAR_REL=...)
#endif
#define MINVAL_F 1e-15f
#define MINIMP_F 1e-4f
#define MAXIMP_F 0.9999f
#define EPS_F 1.1920929e-7f

// ------------------------------------------------------------------ small math
DEV float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
DEV void cross3(float* o, const float* a, const float* b) {
  float x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  o[0] = x; o[1] = y; o[2] = z;
}
DEV float normalize3(float* a) {
  float n = sqrtf(dot3(a, a));
  if (n < MINVAL_F) { a[0] = 1.f; a[1] = 0.f; a[2] = 0.f; return 0.f; }
  float inv = 1.f / n;
  a[0] *= inv; a[1] *= inv; a[2] *= inv;
  return n;
}
DEV void matvec3(float* o, const float* m, const float* v) {
  float x = m[0] * v[0] + m[1] * v[1] + m[2] * v[2];
  float y = m[3] * v[0] + m[4] * v[1] + m[5] * v[2];
  float z = m[6] * v[0] + m[7] * v[1] + m[8] * v[2];
  o[0] = x; o[1] = y; o[2] = z;
}
DEV void matTvec3(float* o, const float* m, const float* v) {
  float x = m[0] * v[0] + m[3] * v[1] + m[6] * v[2];
  float y = m[1] * v[0] + m[4] * v[1] + m[7] * v[2];
  float z = m[2] * v[0] + m[5] * v[1] + m[8] * v[2];
  o[0] = x; o[1] = y; o[2] = z;
}
DEV void matmul3(float* o, const float* a, const float* b) {
  float t[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) t[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
#pragma unroll
  for (int i = 0; i < 9; i++) o[i] = t[i];
}
DEV void quat2mat(float* m, const float* q) {
  float w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = 1.f - 2.f * (y * y + z * z); m[1] = 2.f * (x * y - w * z); m[2] = 2.f * (x * z + w * y);
  m[3] = 2.f * (x * y + w * z); m[4] = 1.f - 2.f * (x * x + z * z); m[5] = 2.f * (y * z - w * x);
  m[6] = 2.f * (x * z - w * y); m[7] = 2.f * (y * z + w * x); m[8] = 1.f - 2.f * (x * x + y * y);
}
DEV void mulquat(float* o, const float* a, const float* b) {
  float w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  float x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  float y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  float z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  o[0] = w; o[1] = x; o[2] = y; o[3] = z;
}
DEV void normquat(float* q) {
  float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (n < MINVAL_F) { q[0] = 1.f; q[1] = q[2] = q[3] = 0.f; return; }
  float inv = 1.f / n;
  q[0] *= inv; q[1] *= inv; q[2] *= inv; q[3] *= inv;
}
// sin and cos of one angle: Cody-Waite reduction by pi/2 (three constants, exact products through fma) and the
// cephes minimax polynomials on [-pi/4, pi/4]; <= 2 ulp for |x| < 1e4 rad (measured 1.52 / 1.55 on 10^6 inputs,
// tests/blocks_cases.py check_sincos), sin(-0) = -0.  The libm sinf/cosf expand to ~220 instructions each
// (large-argument path), and the kinematics needs six pairs per substep.
DEV void sincos_f(float x, float* sn, float* cs) {
  float k = rintf(x * 0.63661977236758134308f);
  float r = fmaf(-k, 1.57079625129699707031f, x);
  r = fmaf(-k, 7.54978941586159635335e-08f, r);
  r = fmaf(-k, 5.39030285815811905290e-15f, r);
  float z = r * r;
  float s = fmaf(r * z, fmaf(z, fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f), -1.6666654611e-1f), r);
  float c = fmaf(z * z, fmaf(z, fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f), 4.166664568298827e-2f), fmaf(-0.5f, z, 1.f));
  s = x == 0.f ? x : s;            // sin(-0) = -0: the reduction and the polynomial both end in (+0) + (-0) = +0
  int q = (int)k;
  float s1 = (q & 1) ? c : s, c1 = (q & 1) ? s : c;
  *sn = (q & 2) ? -s1 : s1;
  *cs = ((q + 1) & 2) ? -c1 : c1;
}
DEV void rotvecquat(float* o, const float* v, const float* q) {
  float m[9]; quat2mat(m, q); matvec3(o, m, v);
}
DEV void mat2quat(float* q, const float* m) {
  float t = m[0] + m[4] + m[8];
  if (t > 0.f) {
    float s = sqrtf(t + 1.f) * 2.f; q[0] = 0.25f * s; q[1] = (m[7] - m[5]) / s; q[2] = (m[2] - m[6]) / s; q[3] = (m[3] - m[1]) / s;
  } else if (m[0] > m[4] && m[0] > m[8]) {
    float s = sqrtf(1.f + m[0] - m[4] - m[8]) * 2.f; q[0] = (m[7] - m[5]) / s; q[1] = 0.25f * s; q[2] = (m[1] + m[3]) / s; q[3] = (m[2] + m[6]) / s;
  } else if (m[4] > m[8]) {
    float s = sqrtf(1.f + m[4] - m[0] - m[8]) * 2.f; q[0] = (m[2] - m[6]) / s; q[1] = (m[1] + m[3]) / s; q[2] = 0.25f * s; q[3] = (m[5] + m[7]) / s;
  } else {
    float s = sqrtf(1.f + m[8] - m[0] - m[4]) * 2.f; q[0] = (m[3] - m[1]) / s; q[1] = (m[2] + m[6]) / s; q[2] = (m[5] + m[7]) / s; q[3] = 0.25f * s;
  }
  normquat(q);
}
// symmetric 3x3 packed as xx yy zz xy xz yz
DEV void symvec3(float* o, const float* s, const float* v) {
  float x = s[0] * v[0] + s[3] * v[1] + s[4] * v[2];
  float y = s[3] * v[0] + s[1] * v[1] + s[5] * v[2];
  float z = s[4] * v[0] + s[5] * v[1] + s[2] * v[2];
  o[0] = x; o[1] = y; o[2] = z;
}
// o = R * S * R^T for symmetric S
DEV void rotsym(float* o, const float* R, const float* s) {
  float t[9];   // t = R*S
#pragma unroll
  for (int i = 0; i < 3; i++) {
    t[3 * i + 0] = R[3 * i] * s[0] + R[3 * i + 1] * s[3] + R[3 * i + 2] * s[4];
    t[3 * i + 1] = R[3 * i] * s[3] + R[3 * i + 1] * s[1] + R[3 * i + 2] * s[5];
    t[3 * i + 2] = R[3 * i] * s[4] + R[3 * i + 1] * s[5] + R[3 * i + 2] * s[2];
  }
  o[0] = t[0] * R[0] + t[1] * R[1] + t[2] * R[2];
  o[1] = t[3] * R[3] + t[4] * R[4] + t[5] * R[5];
  o[2] = t[6] * R[6] + t[7] * R[7] + t[8] * R[8];
  o[3] = t[0] * R[3] + t[1] * R[4] + t[2] * R[5];
  o[4] = t[0] * R[6] + t[1] * R[7] + t[2] * R[8];
  o[5] = t[3] * R[6] + t[4] * R[7] + t[5] * R[8];
}
DEV int tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// ------------------------------------------------------------------ solimp impedance
// x^power for the solimp sigmoid with a power other than MuJoCo's default 2: ONE out-of-line copy (the inlined
// ocml powf is ~1100 instructions and impedance() is expanded at three call sites)
static __device__ __attribute__((noinline)) float impedance_pow(float x, float power) { return powf(x, power); }

DEV float impedance(const float* solimp, float pos) {
  float dmin = fminf(fmaxf(solimp[0], MINIMP_F), MAXIMP_F), dmax = fminf(fmaxf(solimp[1], MINIMP_F), MAXIMP_F);
  float width = fmaxf(solimp[2], 0.f), mid = fminf(fmaxf(solimp[3], MINIMP_F), MAXIMP_F), power = fmaxf(solimp[4], 1.f);
  if (dmin == dmax || width <= MINVAL_F) return 0.5f * (dmin + dmax);
  float x = fabsf(pos) / width;
  if (x >= 1.f) return dmax;
  if (x <= 0.f) return dmin;
  float y;
  if (power == 1.f) y = x;
  else if (power == 2.f) y = x <= mid ? x * x / mid : 1.f - (1.f - x) * (1.f - x) / (1.f - mid);
  else if (x <= mid) y = impedance_pow(x, power) / impedance_pow(mid, power - 1.f);
  else y = 1.f - impedance_pow(1.f - x, power) / impedance_pow(1.f - mid, power - 1.f);
  return dmin + y * (dmax - dmin);
}

// ------------------------------------------------------------------ oriented boxes (overlap reward: so100_hand_over.py:238-275)
struct BoxW { float pos[3], quat[4], half[3]; };

DEV bool overlap_aabb_oobb(const float* half0, const BoxW& b) {
  float R[9]; quat2mat(R, b.quat);
  // 6 face axes only, strict inequalities (oobb_utils.py:223-246); projections of the 8 corners reduce to centre +- extent
  bool sep = false;
#pragma unroll
  for (int a = 0; a < 6; a++) {
    float ax[3];
    if (a < 3) { ax[0] = a == 0; ax[1] = a == 1; ax[2] = a == 2; }
    else { ax[0] = R[a - 3]; ax[1] = R[3 + a - 3]; ax[2] = R[6 + a - 3]; }
    float mx0 = -3e38f, mn0 = 3e38f, mx1 = -3e38f, mn1 = 3e38f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      float sx = (i & 1) ? 1.f : -1.f, sy = (i & 2) ? 1.f : -1.f, sz = (i & 4) ? 1.f : -1.f;
      float av[3] = {sx * half0[0], sy * half0[1], sz * half0[2]};
      float lv[3] = {sx * b.half[0], sy * b.half[1], sz * b.half[2]}, ov[3];
      matvec3(ov, R, lv);
      ov[0] += b.pos[0]; ov[1] += b.pos[1]; ov[2] += b.pos[2];
      float p0 = dot3(av, ax), p1 = dot3(ov, ax);
      mx0 = fmaxf(mx0, p0); mn0 = fminf(mn0, p0); mx1 = fmaxf(mx1, p1); mn1 = fminf(mn1, p1);
    }
    if (mx0 < mn1 || mn0 > mx1) sep = true;
  }
  return !sep;
}

DEV bool overlap_oobb_oobb(const BoxW& b0, const BoxW& b1) {
  float inv[4] = {b0.quat[0], -b0.quat[1], -b0.quat[2], -b0.quat[3]};
  float dp[3] = {b1.pos[0] - b0.pos[0], b1.pos[1] - b0.pos[1], b1.pos[2] - b0.pos[2]};
  BoxW r;
  rotvecquat(r.pos, dp, inv);
  mulquat(r.quat, inv, b1.quat);
  r.half[0] = b1.half[0]; r.half[1] = b1.half[1]; r.half[2] = b1.half[2];
  return overlap_aabb_oobb(b0.half, r);
}

// ------------------------------------------------------------------ counter RNG (Philox4x32-10), 24-bit uniforms
DEV float rng_uniform(unsigned long long seed, unsigned long long env, unsigned int episode, unsigned int draw) {
  unsigned int c0 = (unsigned int)env, c1 = (unsigned int)(env >> 32), c2 = episode, c3 = draw;
  unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; r++) {
    unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned int)p1, n2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned int)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return (float)(c0 >> 8) * (1.0f / 16777216.0f);
}
