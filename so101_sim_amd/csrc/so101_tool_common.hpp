// Chain-independent pieces of Cartesian tool control (the kernels: so101_tool_chain.hpp): the limit clamp, the rotation vector, the orientation error of the three modes and the damped least-squares step,
// templated on the number of joint columns.  The algorithm they belong to is written down in include/so101.h (so101_tool_ik).
#pragma once
#include "so101_math.hpp"

DEV float tool_clamp(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// rotation vector (axis times angle, angle in [0, pi]) from v = sin(angle) axis and c = cos(angle).  At sin(angle) = 0 the axis is undefined: the
// result is v itself (zero) for c > 0, and pi times `fallback` (a unit vector the caller chose) at an angle of pi.
DEV void tool_rotvec(float* o, const float* v, float c, const float* fallback) {
  const float s = sqrtf(dot3(v, v));
  if (s > 1e-12f) {
    const float k = atan2f(s, c) / s;
    o[0] = k * v[0]; o[1] = k * v[1]; o[2] = k * v[2];
  } else if (c > 0.f) {
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
  } else {
    const float pi = 3.14159265358979323846f;
    o[0] = pi * fallback[0]; o[1] = pi * fallback[1]; o[2] = pi * fallback[2];
  }
}

// orientation error of the modes (include/so101.h).  The axis chosen at an angle of exactly pi:
//   mode 1: z x e_k normalised, e_k the coordinate axis along which |z| is smallest (the lowest k on ties) - a unit vector across z;
//   mode 2: the column of R + I (R = M_target M^T) with the largest diagonal entry (the lowest on ties), normalised.
DEV void tool_rot_error(int mode, const float* M, const float* Mt, float* er) {
  er[0] = er[1] = er[2] = 0.f;
  if (mode == 1) {
    const float z[3] = {M[2], M[5], M[8]}, zt[3] = {Mt[2], Mt[5], Mt[8]};
    float v[3]; cross3(v, z, zt);
    const float ax = fabsf(z[0]), ay = fabsf(z[1]), az = fabsf(z[2]);
    float ek[3] = {0.f, 0.f, 0.f};
    if (ax <= ay && ax <= az) ek[0] = 1.f; else if (ay <= az) ek[1] = 1.f; else ek[2] = 1.f;
    float fb[3]; cross3(fb, z, ek); normalize3(fb);
    tool_rotvec(er, v, dot3(z, zt), fb);
  } else if (mode == 2) {
    float R[9];                        // R = Mt M^T
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) R[3 * i + j] = Mt[3 * i] * M[3 * j] + Mt[3 * i + 1] * M[3 * j + 1] + Mt[3 * i + 2] * M[3 * j + 2];
    const float v[3] = {0.5f * (R[7] - R[5]), 0.5f * (R[2] - R[6]), 0.5f * (R[3] - R[1])};
    const float c = 0.5f * (R[0] + R[4] + R[8] - 1.f);
    float fb[3];
    if (R[0] >= R[4] && R[0] >= R[8]) { fb[0] = R[0] + 1.f; fb[1] = R[3]; fb[2] = R[6]; }
    else if (R[4] >= R[8]) { fb[0] = R[1]; fb[1] = R[4] + 1.f; fb[2] = R[7]; }
    else { fb[0] = R[2]; fb[1] = R[5]; fb[2] = R[8] + 1.f; }
    normalize3(fb);
    tool_rotvec(er, v, c, fb);
  }
}

// dq = Jw^T (Jw Jw^T + lambda I)^-1 e over NC joint columns, with Jw = [Jp ; w Jr'], e = [e_p ; w e_r], lambda = e . e + damping: the 6 x 6 system is factored by an
// unpivoted Cholesky in registers.  lambda > 0 makes the matrix positive definite; a pivot that rounds to nothing is raised to MINVAL_F.
template <int NC>
DEV void tool_dls_step(int mode, float w, float damping, const float* M, float (*Jp)[3], float (*Jr)[3], const float* ep, const float* er, float* dq) {
  float Jw[6][NC];                   // [row][joint]
  const float z[3] = {M[2], M[5], M[8]};
#pragma unroll
  for (int j = 0; j < NC; j++) {
    float r[3] = {0.f, 0.f, 0.f};
    if (mode == 1) {
      const float d = dot3(z, Jr[j]);
#pragma unroll
      for (int i = 0; i < 3; i++) r[i] = Jr[j][i] - z[i] * d;
    } else if (mode == 2) {
#pragma unroll
      for (int i = 0; i < 3; i++) r[i] = Jr[j][i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) { Jw[i][j] = Jp[j][i]; Jw[3 + i][j] = w * r[i]; }
  }
  float e[6] = {ep[0], ep[1], ep[2], w * er[0], w * er[1], w * er[2]};
  float lambda = damping;
#pragma unroll
  for (int i = 0; i < 6; i++) lambda += e[i] * e[i];
  float A[6][6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int k = 0; k <= i; k++) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < NC; j++) s += Jw[i][j] * Jw[k][j];
      A[i][k] = i == k ? s + lambda : s;
    }
  }
  // A = L L^T in place (lower triangle), the inverse of the diagonal kept for the two substitutions
  float dinv[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int k = 0; k < i; k++) {
      float s = A[i][k];
#pragma unroll
      for (int l = 0; l < k; l++) s -= A[i][l] * A[k][l];
      A[i][k] = s * dinv[k];
    }
    float d = A[i][i];
#pragma unroll
    for (int l = 0; l < i; l++) d -= A[i][l] * A[i][l];
    d = sqrtf(fmaxf(d, MINVAL_F));
    A[i][i] = d; dinv[i] = 1.f / d;
  }
  float y[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    float s = e[i];
#pragma unroll
    for (int l = 0; l < i; l++) s -= A[i][l] * y[l];
    y[i] = s * dinv[i];
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    float s = y[i];
#pragma unroll
    for (int l = i + 1; l < 6; l++) s -= A[l][i] * y[l];
    y[i] = s * dinv[i];
  }
#pragma unroll
  for (int j = 0; j < NC; j++) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 6; i++) s += Jw[i][j] * y[i];
    dq[j] = s;
  }
}
