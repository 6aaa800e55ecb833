// Device code of the batched SO100 hand-over step: ONE ENVIRONMENT PER WAVEFRONT (64 lanes).
//
// Stages per physics substep (MuJoCo mj_step order; the reference drives 10 of them per env.step,
// so101_sim/task_suite.py:41):
//   kinematics -> CRBA (arm 6x6) + inverse -> RNE bias -> actuation -> smooth acceleration
//   -> geom AABBs -> broadphase over the statically filtered pair list -> MPR narrowphase with
//   wave-parallel hull support -> constraint rows (dof frictionloss, joint limits, elliptic contacts)
//   -> PGS in velocity space -> semi-implicit Euler.
// Lane use: "uniform" code is executed identically by all lanes on wave-uniform values; "lane-
// parallel" code maps lanes to dofs / geoms / pairs / contacts / hull vertices.  All cross-lane data
// flows through LDS (EnvLDS) between wave_sync() points or through the helpers in wave.hpp.
//
// Free bodies are carried in centre-of-mass twist coordinates inside the solver (inverse inertia is
// then 1/m and a symmetric 3x3), and mapped back to MuJoCo's (origin velocity, body-frame angular
// velocity) coordinates for integration; the PGS force iterates are invariant to that change of
// velocity coordinates.
//
// What both engines share lives in so101_math.hpp (small math) and so101_geom.hpp (the whole narrowphase); this file is the SO100 engine:
// everything below works on EnvLDS.
#pragma once
#include "so101_model.hpp"
#include "wave.hpp"
#include "so101_geom.hpp"

// world inertia of every dynamic body (lane-parallel)
DEV void world_inertias(const DevModel* m, EnvLDS& L) {
  int lane = wave_lane();
  if (lane < NDYN) {
    const float* Ib = lane < NARM ? m->arm_Ib[lane] : m->free_Ib[lane - NARM];
    float sc = lane < NARM ? 1.f : L.fscale[lane - NARM];      // per-env prop mass scale: mass and inertia scale together
    float o[6]; rotsym(o, L.xmat[lane], Ib);
#pragma unroll
    for (int i = 0; i < 6; i++) L.Iw[lane][i] = sc * o[i];
    if (lane >= NARM) {
      int f = lane - NARM;
      float oi[6]; rotsym(oi, L.xmat[lane], m->free_Ibinv[f]);
      float isc = 1.f / sc;
#pragma unroll
      for (int i = 0; i < 6; i++) L.fIinv[f][i] = isc * oi[i];
      L.fmass[f] = sc * m->free_mass[f];
      L.fminv[f] = 1.f / L.fmass[f];
    }
  }
  wave_sync();
}

// ------------------------------------------------------------------ kinematics (uniform)
DEV void kinematics(const DevModel* m, EnvLDS& L) {
  int lane = wave_lane();
  // arm chain: every lane walks the 6 links on uniform values; lane 0 publishes to LDS
  float xp[3] = {m->base_pos[0], m->base_pos[1], m->base_pos[2]};
  float xq[4] = {m->base_quat[0], m->base_quat[1], m->base_quat[2], m->base_quat[3]};
  float R[9]; quat2mat(R, xq);
#pragma unroll
  for (int k = 0; k < NARM; k++) {
    float t[3]; matvec3(t, R, m->arm_pos[k]);
    xp[0] += t[0]; xp[1] += t[1]; xp[2] += t[2];
    mulquat(xq, xq, m->arm_quat[k]);
    float sn, cs; sincos_f(0.5f * L.qpos[k], &sn, &cs);
    float jq[4] = {cs, m->arm_axis[k][0] * sn, m->arm_axis[k][1] * sn, m->arm_axis[k][2] * sn};
    mulquat(xq, xq, jq);
    normquat(xq);
    quat2mat(R, xq);
    float ax[3]; matvec3(ax, R, m->arm_axis[k]);
    float ip[3]; matvec3(ip, R, m->arm_ipos[k]);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 3; i++) { L.xpos[k][i] = xp[i]; L.axis[k][i] = ax[i]; L.xipos[k][i] = xp[i] + ip[i]; }
#pragma unroll
      for (int i = 0; i < 9; i++) L.xmat[k][i] = R[i];
    }
  }
  // free bodies: lanes 0..NFREE-1
  if (lane < NFREE) {
    int f = lane, b = NARM + f;
    const float* q = &L.qpos[NARM + 7 * f];
    float fq[4] = {q[3], q[4], q[5], q[6]};
    normquat(fq);
    float Rf[9]; quat2mat(Rf, fq);
    float ip[3]; matvec3(ip, Rf, m->free_ipos[f]);
#pragma unroll
    for (int i = 0; i < 3; i++) { L.xpos[b][i] = q[i]; L.xipos[b][i] = q[i] + ip[i]; }
#pragma unroll
    for (int i = 0; i < 9; i++) L.xmat[b][i] = Rf[i];
  }
  wave_sync();
  world_inertias(m, L);
}

// Kinematics of a state whose body poses are already known (the pipelined step publishes them for the narrowphase at
// the end of the previous kernel): poses from global memory, then the derived quantities one body per lane - joint axes,
// COM positions, world inertias - with the same expressions kinematics() uses, so the bits are the same.  Replaces the
// serial walk down the arm (every lane on identical values, ~900 dependent instructions) by ~50.
template <bool AG = false>       // AG: the poses were stored by another wavefront of this launch (wave.hpp, agent-scope loads)
DEV void kinematics_from_pose(const DevModel* m, EnvLDS& L, const float* pose /* [NDYN][12]: xpos, xmat */) {
  int lane = wave_lane();
  for (int i = lane; i < NDYN * 12; i += WAVE) {
    int b = i / 12, j = i % 12;
    float v = AG ? ld_agent(&pose[i]) : pose[i];
    if (j < 3) L.xpos[b][j] = v; else L.xmat[b][j - 3] = v;
  }
  wave_sync();
  if (lane < NARM) {
    int k = lane;
    float R[9];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = L.xmat[k][i];
    float ax[3]; matvec3(ax, R, m->arm_axis[k]);
    float ip[3]; matvec3(ip, R, m->arm_ipos[k]);
#pragma unroll
    for (int i = 0; i < 3; i++) { L.axis[k][i] = ax[i]; L.xipos[k][i] = L.xpos[k][i] + ip[i]; }
  } else if (lane < NDYN) {
    int f = lane - NARM, b = lane;
    float Rf[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Rf[i] = L.xmat[b][i];
    float ip[3]; matvec3(ip, Rf, m->free_ipos[f]);
#pragma unroll
    for (int i = 0; i < 3; i++) L.xipos[b][i] = L.xpos[b][i] + ip[i];
  }
  wave_sync();
  world_inertias(m, L);
}

// ------------------------------------------------------------------ CRBA + inverse of the arm block
DEV void crba_arm(const DevModel* m, EnvLDS& L) {
  int lane = wave_lane();
  // composite (mass, COM, inertia about COM) of the sub-chain k..5 — uniform backward pass
  float mc[NARM], Cc[NARM][3], Ic[NARM][6];
  float cm = 0.f, cC[3] = {0.f, 0.f, 0.f}, cI[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = NARM - 1; k >= 0; k--) {
    float m1 = m->arm_mass[k], mt = m1 + cm;
    float c1[3] = {L.xipos[k][0], L.xipos[k][1], L.xipos[k][2]};
    float C[3];
#pragma unroll
    for (int i = 0; i < 3; i++) C[i] = (m1 * c1[i] + cm * cC[i]) / mt;
    float d1[3] = {c1[0] - C[0], c1[1] - C[1], c1[2] - C[2]};
    float d2[3] = {cC[0] - C[0], cC[1] - C[1], cC[2] - C[2]};
    float dd1 = dot3(d1, d1), dd2 = dot3(d2, d2);
    float I[6];
    I[0] = L.Iw[k][0] + cI[0] + m1 * (dd1 - d1[0] * d1[0]) + cm * (dd2 - d2[0] * d2[0]);
    I[1] = L.Iw[k][1] + cI[1] + m1 * (dd1 - d1[1] * d1[1]) + cm * (dd2 - d2[1] * d2[1]);
    I[2] = L.Iw[k][2] + cI[2] + m1 * (dd1 - d1[2] * d1[2]) + cm * (dd2 - d2[2] * d2[2]);
    I[3] = L.Iw[k][3] + cI[3] - m1 * d1[0] * d1[1] - cm * d2[0] * d2[1];
    I[4] = L.Iw[k][4] + cI[4] - m1 * d1[0] * d1[2] - cm * d2[0] * d2[2];
    I[5] = L.Iw[k][5] + cI[5] - m1 * d1[1] * d1[2] - cm * d2[1] * d2[2];
    cm = mt;
#pragma unroll
    for (int i = 0; i < 3; i++) cC[i] = C[i];
#pragma unroll
    for (int i = 0; i < 6; i++) cI[i] = I[i];
    mc[k] = cm;
#pragma unroll
    for (int i = 0; i < 3; i++) Cc[k][i] = cC[i];
#pragma unroll
    for (int i = 0; i < 6; i++) Ic[k][i] = cI[i];
  }
  // M[j][k], k <= j: lane e computes entry e of the packed lower triangle (21 entries) from the composites, which lane 0
  // parks in LDS (the Newton scratch is idle here).  Every lane used to compute all 21 entries on identical values.
  float* park = &L.nw.H[0][0];                       // [NARM][10]: mass, COM, inertia of sub-chain j..5
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < NARM; j++) {
      park[10 * j] = mc[j];
#pragma unroll
      for (int i = 0; i < 3; i++) park[10 * j + 1 + i] = Cc[j][i];
#pragma unroll
      for (int i = 0; i < 6; i++) park[10 * j + 4 + i] = Ic[j][i];
    }
  }
  wave_sync();
  if (lane < NARM * (NARM + 1) / 2) {
    int j = 0;
#pragma unroll
    for (int t = 1; t < NARM; t++) j += lane >= t * (t + 1) / 2 ? 1 : 0;
    int k = lane - j * (j + 1) / 2;
    const float* pj = park + 10 * j;
    float mcj = pj[0], Ccj[3] = {pj[1], pj[2], pj[3]}, Icj[6] = {pj[4], pj[5], pj[6], pj[7], pj[8], pj[9]};
    float ak[3] = {L.axis[k][0], L.axis[k][1], L.axis[k][2]};
    float aj[3] = {L.axis[j][0], L.axis[j][1], L.axis[j][2]};
    float rk[3] = {Ccj[0] - L.xpos[k][0], Ccj[1] - L.xpos[k][1], Ccj[2] - L.xpos[k][2]};
    float rj[3] = {Ccj[0] - L.xpos[j][0], Ccj[1] - L.xpos[j][1], Ccj[2] - L.xpos[j][2]};
    float hl[3]; cross3(hl, ak, rk);
    hl[0] *= mcj; hl[1] *= mcj; hl[2] *= mcj;
    float ha[3]; symvec3(ha, Icj, ak);
    float t3[3]; cross3(t3, rj, hl);
    float v = aj[0] * (ha[0] + t3[0]) + aj[1] * (ha[1] + t3[1]) + aj[2] * (ha[2] + t3[2]);
    if (j == k) v += m->armature[j];
    L.Marm[j][k] = v; L.Marm[k][j] = v;
  }
  wave_sync();
  float Mfull[NARM][NARM];
#pragma unroll
  for (int j = 0; j < NARM; j++)
#pragma unroll
    for (int k = 0; k <= j; k++) { float v = L.Marm[j][k]; Mfull[j][k] = v; Mfull[k][j] = v; }
  // Cholesky (uniform) then lane c solves for column c of the inverse
  float Lc[NARM][NARM];
#pragma unroll
  for (int j = 0; j < NARM; j++) {
    float d = Mfull[j][j];
#pragma unroll
    for (int k = 0; k < j; k++) d -= Lc[j][k] * Lc[j][k];
    d = sqrtf(d);
    Lc[j][j] = d;
    float inv = 1.f / d;
#pragma unroll
    for (int i = j + 1; i < NARM; i++) {
      float v = Mfull[i][j];
#pragma unroll
      for (int k = 0; k < j; k++) v -= Lc[i][k] * Lc[j][k];
      Lc[i][j] = v * inv;
    }
  }
  if (lane < NARM) {
    float y[NARM], x[NARM];
#pragma unroll
    for (int i = 0; i < NARM; i++) {
      float v = (i == lane) ? 1.f : 0.f;
#pragma unroll
      for (int k = 0; k < i; k++) v -= Lc[i][k] * y[k];
      y[i] = v / Lc[i][i];
    }
#pragma unroll
    for (int i = NARM - 1; i >= 0; i--) {
      float v = y[i];
#pragma unroll
      for (int k = i + 1; k < NARM; k++) v -= Lc[k][i] * x[k];
      x[i] = v / Lc[i][i];
    }
#pragma unroll
    for (int i = 0; i < NARM; i++) L.Minv[i][lane] = x[i];
  }
  wave_sync();
}

// ------------------------------------------------------------------ RNE bias, actuation, smooth acceleration
DEV void smooth_dynamics(const DevModel* m, EnvLDS& L) {
  int lane = wave_lane();
  // --- arm: recursive Newton-Euler with zero joint acceleration and gravity as base acceleration
  float w[3] = {0.f, 0.f, 0.f}, al[3] = {0.f, 0.f, 0.f}, ao[3] = {-m->grav[0], -m->grav[1], -m->grav[2]};
  float pp[3] = {m->base_pos[0], m->base_pos[1], m->base_pos[2]};
  float fk[NARM][3], nk[NARM][3];
#pragma unroll
  for (int k = 0; k < NARM; k++) {
    float d[3] = {L.xpos[k][0] - pp[0], L.xpos[k][1] - pp[1], L.xpos[k][2] - pp[2]};
    float t1[3], t2[3];
    cross3(t1, al, d); cross3(t2, w, d); cross3(t2, w, t2);
    ao[0] += t1[0] + t2[0]; ao[1] += t1[1] + t2[1]; ao[2] += t1[2] + t2[2];
    float a[3] = {L.axis[k][0], L.axis[k][1], L.axis[k][2]};
    float qd = L.qvel[k];
    float wa[3]; cross3(wa, w, a);
    al[0] += wa[0] * qd; al[1] += wa[1] * qd; al[2] += wa[2] * qd;
    w[0] += a[0] * qd; w[1] += a[1] * qd; w[2] += a[2] * qd;
    float r[3] = {L.xipos[k][0] - L.xpos[k][0], L.xipos[k][1] - L.xpos[k][1], L.xipos[k][2] - L.xpos[k][2]};
    cross3(t1, al, r); cross3(t2, w, r); cross3(t2, w, t2);
    float mass = m->arm_mass[k];
    float F[3] = {mass * (ao[0] + t1[0] + t2[0]), mass * (ao[1] + t1[1] + t2[1]), mass * (ao[2] + t1[2] + t2[2])};
    float Iw_[3], Ia[3], N[3], rF[3];
    symvec3(Iw_, L.Iw[k], w); symvec3(Ia, L.Iw[k], al);
    cross3(N, w, Iw_); cross3(rF, r, F);
#pragma unroll
    for (int i = 0; i < 3; i++) { fk[k][i] = F[i]; nk[k][i] = Ia[i] + N[i] + rF[i]; pp[i] = L.xpos[k][i]; }
  }
  float bias[NARM];
#pragma unroll
  for (int k = NARM - 1; k >= 0; k--) {
    bias[k] = L.axis[k][0] * nk[k][0] + L.axis[k][1] * nk[k][1] + L.axis[k][2] * nk[k][2];
    if (k > 0) {
      float dd[3] = {L.xpos[k][0] - L.xpos[k - 1][0], L.xpos[k][1] - L.xpos[k - 1][1], L.xpos[k][2] - L.xpos[k - 1][2]};
      float t[3]; cross3(t, dd, fk[k]);
#pragma unroll
      for (int i = 0; i < 3; i++) { fk[k - 1][i] += fk[k][i]; nk[k - 1][i] += nk[k][i] + t[i]; }
    }
  }
  // --- actuation (lane = actuator = dof for this model): clamp ctrl, affine bias, clamp force
  if (lane < NARM) {
    float c = L.ctrl[lane];
    if (m->ctrllimited[lane]) c = fminf(fmaxf(c, m->ctrlrange[lane][0]), m->ctrlrange[lane][1]);
    float force = m->act_gain[lane] * c + m->act_bias[lane][0] + m->act_bias[lane][1] * L.qpos[lane] + m->act_bias[lane][2] * L.qvel[lane];
    if (m->forcelimited[lane]) force = fminf(fmaxf(force, m->forcerange[lane][0]), m->forcerange[lane][1]);
    float b = 0.f;
#pragma unroll
    for (int k = 0; k < NARM; k++) if (k == lane) b = bias[k];
    L.bias[lane] = b;
    L.tau[lane] = force - b;
  }
  wave_sync();
  if (lane < NARM) {
    float v = 0.f;
#pragma unroll
    for (int c = 0; c < NARM; c++) v += L.Minv[lane][c] * L.tau[c];
    L.qacc_arm[lane] = v;
  }
  // --- free bodies in COM-twist coordinates: a_com = g, alpha = Iinv (-w x I w)
  if (lane >= 32 && lane < 32 + NFREE) {
    int f = lane - 32, b = NARM + f;
    const float* qv = &L.qvel[NARM + 6 * f];
    float wb[3] = {qv[3], qv[4], qv[5]}, ww[3];
    matvec3(ww, L.xmat[b], wb);
    float r[3] = {L.xipos[b][0] - L.xpos[b][0], L.xipos[b][1] - L.xpos[b][1], L.xipos[b][2] - L.xpos[b][2]};
    float wr[3]; cross3(wr, ww, r);
    float Iw_[3]; symvec3(Iw_, L.Iw[b], ww);
    float g[3]; cross3(g, ww, Iw_);
    g[0] = -g[0]; g[1] = -g[1]; g[2] = -g[2];
    float alp[3]; symvec3(alp, L.fIinv[f], g);
    // Solver coordinates: (a~, alpha) with a~ = qacc_lin + alpha x r, i.e. the COM acceleration WITHOUT the
    // centripetal term w x (w x r).  J*qacc in MuJoCo's generalized coordinates (which neglects Jdot*qvel)
    // is then e.(a~ + alpha x (p - com)) exactly, and force updates stay (1/m, Iinv).
    float cen[3]; cross3(cen, ww, wr);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      L.fvel[f][i] = qv[i] + wr[i]; L.fvel[f][3 + i] = ww[i];
      L.facc[f][i] = m->grav[i] - cen[i]; L.facc[f][3 + i] = alp[i];
    }
  }
  wave_sync();
}

// ------------------------------------------------------------------ geoms of an env (so101_geom.hpp with the poses in LDS)
DEV void load_geom(const DevModel* m, const EnvLDS& L, int g, GeomW& G) {
  g = wave_uniform_i(g);
  int d = ldc(ldc(&m->geom_dyn) + g);
  load_geom_at(m, g, L.xpos[d < 0 ? 0 : d], L.xmat[d < 0 ? 0 : d], G);
}

// ------------------------------------------------------------------ collision driver
// oriented box of geom g in the world: axes R (columns), centre c, half extents h (the geom-frame box that the model
// compiler put around the hull / primitive)
DEV void geom_obb(const DevModel* m, const EnvLDS& L, int g, float* R, float* c, float* h) {
  const float* ab = m->geom_aabb + 6 * g;
  const float* gp = m->geom_pos + 3 * g; const float* gm = m->geom_mat + 9 * g;
  int d = m->geom_dyn[g];
  float lm[9], lp[3] = {gp[0], gp[1], gp[2]}, p[3];
#pragma unroll
  for (int i = 0; i < 9; i++) lm[i] = gm[i];
  if (d < 0) {
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = lm[i];
#pragma unroll
    for (int i = 0; i < 3; i++) p[i] = lp[i];
  } else {
    matmul3(R, L.xmat[d], lm);
    float t[3]; matvec3(t, L.xmat[d], lp);
#pragma unroll
    for (int i = 0; i < 3; i++) p[i] = L.xpos[d][i] + t[i];
  }
  float lc[3] = {ab[0], ab[1], ab[2]}, cw[3];
  matvec3(cw, R, lc);
#pragma unroll
  for (int i = 0; i < 3; i++) { c[i] = p[i] + cw[i]; h[i] = ab[3 + i]; }
}

// Second broadphase pass, lane = candidate: separating-axis test of the two geoms' ORIENTED boxes (15 axes).  The world
// axis-aligned box of a long tilted link overlaps many hulls it is nowhere near; the oriented box is tight.  A pair whose
// oriented boxes are more than 1e-6 m apart cannot touch, so dropping it here changes no contact - it only spares the
// narrowphase a query that would end in "no intersection" (a wavefront's work for a few microseconds; here it costs one
// lane a few hundred instructions).  Plane pairs pass untouched.  The candidate list is compacted in place, order kept.
DEV void obb_filter(const DevModel* m, EnvLDS& L) {
  int lane = wave_lane();
  int ncand = L.ncand, nout = 0;
  for (int k0 = 0; k0 < ncand; k0 += WAVE) {
    int k = k0 + lane;
    bool keep = false; int g1 = 0, g2 = 0;
    if (k < ncand) {
      g1 = L.cand[k][0]; g2 = L.cand[k][1];
      keep = true;
      if (m->geom_type[g1] != G_PLANE) {
        float A[9], ca[3], a[3], B[9], cb[3], b[3];
        geom_obb(m, L, g1, A, ca, a); geom_obb(m, L, g2, B, cb, b);
        // B in A's frame: Rm = A' B, t = A' (cb - ca)
        float Rm[3][3], Ab[3][3], dv[3] = {cb[0] - ca[0], cb[1] - ca[1], cb[2] - ca[2]}, t[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
          t[i] = A[i] * dv[0] + A[3 + i] * dv[1] + A[6 + i] * dv[2];
#pragma unroll
          for (int j = 0; j < 3; j++) {
            Rm[i][j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
            Ab[i][j] = fabsf(Rm[i][j]) + 1e-6f;
          }
        }
        const float gap = 1e-6f;
        bool sep = false;
#pragma unroll
        for (int i = 0; i < 3; i++) sep = sep || fabsf(t[i]) > a[i] + b[0] * Ab[i][0] + b[1] * Ab[i][1] + b[2] * Ab[i][2] + gap;
#pragma unroll
        for (int j = 0; j < 3; j++)
          sep = sep || fabsf(t[0] * Rm[0][j] + t[1] * Rm[1][j] + t[2] * Rm[2][j]) > a[0] * Ab[0][j] + a[1] * Ab[1][j] + a[2] * Ab[2][j] + b[j] + gap;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 3; j++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            float ra = a[i1] * Ab[i2][j] + a[i2] * Ab[i1][j], rb = b[j1] * Ab[i][j2] + b[j2] * Ab[i][j1];
            sep = sep || fabsf(t[i2] * Rm[i1][j] - t[i1] * Rm[i2][j]) > ra + rb + gap;
          }
        keep = !sep;
        if (keep && m->hull_sbt && m->geom_type[g2] == G_MESH) keep = !sbt_separated(m, g1, g2, A, ca, a, B, cb, t);
      } else if (m->hull_sbt && m->geom_type[g2] == G_MESH) {
        // the plane against a hull: the same bound along the plane's normal
        float A[9], ca[3], a[3], B[9], cb[3], b[3];
        geom_obb(m, L, g1, A, ca, a); geom_obb(m, L, g2, B, cb, b);
        float pp[3] = {ca[0], ca[1], ca[2]}, n[3] = {A[2], A[5], A[8]};
        if (m->geom_dyn[g1] < 0) { pp[0] = m->geom_pos[3 * g1]; pp[1] = m->geom_pos[3 * g1 + 1]; pp[2] = m->geom_pos[3 * g1 + 2]; }
        keep = !sbt_plane_separated(m, g2, pp, n, B, cb);
      }
    }
    unsigned long long mask = wave_ballot(keep);
    int idx = nout + wave_prefix(mask);
    wave_sync();                                   // every lane has read its candidate before the slots are rewritten
    if (keep) { L.cand[idx][0] = (unsigned short)g1; L.cand[idx][1] = (unsigned short)g2; }
    nout += __popcll(mask);
  }
  wave_sync();
  if (lane == 0) L.ncand = nout;
  wave_sync();
}

// Broadphase: world boxes of all geoms, then the statically filtered pair list is tested lane-parallel; survivors
// are appended to L.cand in pair order.  The pair words of a chunk (PAIR_CHUNK x 64 pairs) are fetched into registers
// with one burst of loads before any of them is used (the loop used to pay one L2 round trip per 64 pairs), and a
// geom's box is two 16-byte LDS reads.
#define PAIR_CHUNK 32
#ifdef SO101_DEBUG_CLOCKS
#define BPROF(k) { unsigned long long pn_ = SO101_CLOCK(); if (wave_lane() == 0) L.nw.prof[k] = (unsigned int)(pn_ - bp_); bp_ = pn_; }
#else
#define BPROF(k)
#endif
DEV void broadphase(const DevModel* m, EnvLDS& L) {
  int lane = wave_lane();
#ifdef SO101_DEBUG_CLOCKS
  unsigned long long bp_ = SO101_CLOCK();
#endif
  for (int g = lane; g < m->ngeom; g += WAVE) {
    const float* ab = m->geom_aabb + 6 * g;
    const float* gp = m->geom_pos + 3 * g; const float* gm = m->geom_mat + 9 * g;
    int d = m->geom_dyn[g];
    float R[9], p[3];
    if (d < 0) {
#pragma unroll
      for (int i = 0; i < 9; i++) R[i] = gm[i];
#pragma unroll
      for (int i = 0; i < 3; i++) p[i] = gp[i];
    } else {
      float lm[9], lp[3] = {gp[0], gp[1], gp[2]};
#pragma unroll
      for (int i = 0; i < 9; i++) lm[i] = gm[i];
      matmul3(R, L.xmat[d], lm);
      float t[3]; matvec3(t, L.xmat[d], lp);
#pragma unroll
      for (int i = 0; i < 3; i++) p[i] = L.xpos[d][i] + t[i];
    }
    float c[3] = {ab[0], ab[1], ab[2]}, h[3] = {ab[3], ab[4], ab[5]}, cw[3];
    matvec3(cw, R, c);
    float blo[3], bhi[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      float e = fabsf(R[3 * i]) * h[0] + fabsf(R[3 * i + 1]) * h[1] + fabsf(R[3 * i + 2]) * h[2];
      blo[i] = p[i] + cw[i] - e; bhi[i] = p[i] + cw[i] + e;
    }
    if (m->geom_type[g] == G_PLANE) {
      // A plane's "box" is the half space it bounds when its normal is a world axis (the floor): another box reaches the
      // plane iff it overlaps that half space - the same test as "lowest corner below the plane", without a special case
      // in the pair loop.  Any other plane gets all of space (its pairs all go on to the narrowphase).
      float n[3] = {R[2], R[5], R[8]};
#pragma unroll
      for (int i = 0; i < 3; i++) {
        bool axis = fabsf(n[i]) == 1.f;
        blo[i] = (axis && n[i] < 0.f) ? p[i] : -3.0e38f;
        bhi[i] = (axis && n[i] > 0.f) ? p[i] : 3.0e38f;
      }
    }
#pragma unroll
    for (int i = 0; i < 3; i++) { L.aabb[i][g] = blo[i]; L.aabb[3 + i][g] = bhi[i]; }
  }
  if (lane == 0) { L.ncand = 0; L.ncon = 0; L.narmcon = 0; }
  wave_sync();
  BPROF(10)
  int base = 0;
  const unsigned int* pairs = ldc(&m->pair_packed);
  const int npair = ldc(&m->npair);
  for (int c0 = 0; c0 < npair; c0 += PAIR_CHUNK * WAVE) {
    unsigned int w[PAIR_CHUNK];
#pragma unroll
    for (int i = 0; i < PAIR_CHUNK; i++) {
      int p = c0 + i * WAVE + lane;
      w[i] = p < npair ? pairs[p] : 0xffffffffu;
    }
    // Phase 1, reads only: the box tests of the whole chunk, one result bit per pair word.  (With the candidate stores in
    // the same loop every iteration waited for its own LDS round trips - the stores may alias the boxes as far as the
    // compiler knows -: 13.5 us per env-substep for 30 iterations; the candidate order is the same either way.)
    unsigned int hits = 0u;
    BPROF(14)
    // straight-line: no branch inside, so the LDS reads of neighbouring pair words overlap (a padding word tests geom 0
    // against itself and is masked out)
#pragma unroll
    for (int i0 = 0; i0 < PAIR_CHUNK; i0 += 4) {
      if (c0 + i0 * WAVE >= npair) break;            // four pair words per basic block (padding words test geom 0 against itself and are masked out)
#pragma unroll
      for (int i = i0; i < i0 + 4; i++) {
        bool valid = w[i] != 0xffffffffu;
        int g1 = valid ? (int)(w[i] & 0xffu) : 0, g2 = valid ? (int)((w[i] >> 8) & 0xffu) : 0;
        float l1[3] = {L.aabb[0][g1], L.aabb[1][g1], L.aabb[2][g1]}, h1[3] = {L.aabb[3][g1], L.aabb[4][g1], L.aabb[5][g1]};
        float l2[3] = {L.aabb[0][g2], L.aabb[1][g2], L.aabb[2][g2]}, h2[3] = {L.aabb[3][g2], L.aabb[4][g2], L.aabb[5][g2]};
        unsigned int sep = (unsigned int)(l1[0] > h2[0]) | (unsigned int)(l2[0] > h1[0]) | (unsigned int)(l1[1] > h2[1]) |
                           (unsigned int)(l2[1] > h1[1]) | (unsigned int)(l1[2] > h2[2]) | (unsigned int)(l2[2] > h1[2]);
        hits |= (valid && sep == 0u) ? (1u << i) : 0u;
      }
    }
    BPROF(15)
    // Phase 2, stores only: survivors appended in pair order
#pragma unroll
    for (int i = 0; i < PAIR_CHUNK; i++) {
      if (c0 + i * WAVE >= npair) break;
      bool hit = (hits >> i) & 1u;
      unsigned long long mask = wave_ballot(hit);
      if (mask == 0ull) continue;
      int idx = base + wave_prefix(mask);
      if (hit && idx < MAXCAND) { L.cand[idx][0] = (unsigned short)(w[i] & 0xffu); L.cand[idx][1] = (unsigned short)((w[i] >> 8) & 0xffu); }
      base += __popcll(mask);
    }
  }
  if (lane == 0) { L.ncand = base < MAXCAND ? base : MAXCAND; if (base > MAXCAND) L.overflow |= 1; }
  wave_sync();
  BPROF(11)
  obb_filter(m, L);
  BPROF(12)
}

// Contact record of an accepted pair (one lane): frame, body indices, mixed friction / solref / solimp
DEV void contact_init(const DevModel* m, Contact& c, int g1, int g2, float dist, const float* nrm, const float* pos) {
  c.dist = dist;
  float fr[9] = {nrm[0], nrm[1], nrm[2], 0, 0, 0, 0, 0, 0};
  make_frame(fr);
#pragma unroll
  for (int i = 0; i < 9; i++) c.frame[i] = fr[i];
#pragma unroll
  for (int i = 0; i < 3; i++) c.pos[i] = pos[i];
  c.d1 = m->geom_dyn[g1]; c.d2 = m->geom_dyn[g2]; c.g1 = g1; c.g2 = g2;
  int cd1 = m->geom_condim[g1], cd2 = m->geom_condim[g2];
  c.dim = cd1 > cd2 ? cd1 : cd2;
#pragma unroll
  for (int i = 0; i < 3; i++) c.fric[i] = fmaxf(m->geom_friction[3 * g1 + i], m->geom_friction[3 * g2 + i]);
  // solref / solimp mixed with equal weights (solmix = 1 on every geom of these scenes); stash in aref/f
  c.aref[0] = 0.5f * (m->geom_solref[2 * g1] + m->geom_solref[2 * g2]);
  c.aref[1] = 0.5f * (m->geom_solref[2 * g1 + 1] + m->geom_solref[2 * g2 + 1]);
#pragma unroll
  for (int i = 0; i < 5; i++) c.f[i] = 0.5f * (m->geom_solimp[5 * g1 + i] + m->geom_solimp[5 * g2 + i]);
  c.armslot = -1;
}

// Fused collision stage: the wave walks its own candidate list.  (The pipelined step hands the candidates to
// k_narrow instead, one wavefront per candidate.)
// More contacts than MAXCON (round 5; until round 4 the tail of the list was cut off): the env goes over to ONE contact per geom pair - the
// first of each pair's patch: the deepest point of a flat patch, the EPA contact of a hull pair - for this substep, so that no touching pair
// loses its contact; flag 128 (event 7, "contacts_reduced").  Only when the touching PAIRS alone exceed MAXCON is the list cut (flag 2,
// "contact_overflow").  The launch chains' gather_contacts() applies the same rule from the pairs' counts, so both step paths keep the
// same contacts in the same order.
DEV int reduce_contacts(EnvLDS& L, int ncon) {
  int lane = wave_lane(), out = 0;
  wave_sync();
  for (int j = 0; j < ncon; j++) {
    bool first = j == 0 || L.con[j].g1 != L.con[j - 1].g1 || L.con[j].g2 != L.con[j - 1].g2;      // (a pair's contacts are consecutive)
    if (first) {
      if (out != j && lane < (int)(sizeof(Contact) / 4)) ((int*)&L.con[out])[lane] = ((const int*)&L.con[j])[lane];
      out++;
    }
    wave_sync();
  }
  return out;
}
DEV void collision(const DevModel* m, EnvLDS& L) {
  int lane = wave_lane();
  broadphase(m, L);
  int ncand = L.ncand, ncon = 0;
  bool full = false, reduced = false;
  for (int k = 0; k < ncand && !full; k++) {
    int g1 = L.cand[k][0], g2 = L.cand[k][1];
    GeomW G1, G2;
    load_geom(m, L, g1, G1); load_geom(m, L, g2, G2);
    PairContacts pc;
    narrow_pair<NoCache>(m, G1, G2, g1, g2, pc);
    int cnt = __popc(pc.valid);
    if (!reduced && ncon + cnt > MAXCON) {
      if (lane == 0) L.overflow |= 128;
      ncon = reduce_contacts(L, ncon);
      reduced = true;
    }
    bool taken = false;                                // (reduced: the pair's first contact only)
#pragma unroll
    for (int j = 0; j < NCPP; j++) {
      if (((pc.valid >> j) & 1u) && !full && !(reduced && taken)) {
        if (ncon >= MAXCON) { if (lane == 0) L.overflow |= 2; full = true; }
        else { if (lane == 0) contact_init(m, L.con[ncon], g1, g2, pc.dist[j], pc.nrm, pc.pos[j]); ncon++; taken = true; }
      }
    }
  }
  if (lane == 0) L.ncon = ncon;
  wave_sync();
}

// ------------------------------------------------------------------ constraint rows
DEV void kb_from_solref(const DevModel* m, const float* solref_in, const float* solimp, float* K, float* B) {
  float s0 = solref_in[0], s1 = solref_in[1];
  float dmax = fminf(fmaxf(solimp[1], MINIMP_F), MAXIMP_F);
  if (s0 > 0.f) {
    s0 = fmaxf(s0, 2.f * m->dt);     // refsafe
    *K = 1.f / fmaxf(MINVAL_F, dmax * dmax * s0 * s0 * s1 * s1);
    *B = 2.f / fmaxf(MINVAL_F, dmax * s0);
  } else {
    *K = -s0 / fmaxf(MINVAL_F, dmax * dmax);
    *B = -s1 / fmaxf(MINVAL_F, dmax);
  }
}

// Jacobian row of contact axis `u` (translational or rotational) against arm link `link`: out[d], d<=link
DEV void arm_jac_row(const EnvLDS& L, int link, const float* p, const float* u, bool rot, float* out) {
#pragma unroll
  for (int d = 0; d < NARM; d++) {
    float v = 0.f;
    if (d <= link) {
      const float* a = L.axis[d];
      if (rot) v = dot3(u, a);
      else {
        float r[3] = {p[0] - L.xpos[d][0], p[1] - L.xpos[d][1], p[2] - L.xpos[d][2]}, t[3];
        cross3(t, a, r);
        v = dot3(u, t);
      }
    }
    out[d] = v;
  }
}

// row j (0-2 translational, 3-5 rotational, along the contact frame's axes) of an arm-link contact's Jacobian in the six arm dofs:
// J(link of geom2) - J(link of geom1); either side may be static or a free body (link -1: a zero row)
DEV void arm_contact_row(const EnvLDS& L, const Contact& c, int j, float* Jd) {
  int l1 = (c.d1 >= 0 && c.d1 < NARM) ? c.d1 : -1, l2 = (c.d2 >= 0 && c.d2 < NARM) ? c.d2 : -1;
  float Jr[NARM], J1[NARM];
  arm_jac_row(L, l2, c.pos, &c.frame[3 * (j % 3)], j >= 3, Jr);
  arm_jac_row(L, l1, c.pos, &c.frame[3 * (j % 3)], j >= 3, J1);
#pragma unroll
  for (int q = 0; q < NARM; q++) Jd[q] = Jr[q] - J1[q];
}

// Constraint rows of the current contacts: scalar rows (dof frictionloss, joint limits), and per contact the
// regularisers R, the cone parameter mu, the reference accelerations and - for contacts that touch an arm link - the
// joint-space Jacobian rows in the LDS pool.  What only PGS needs (the diagonal blocks of A) is built by solve_pgs().
DEV void make_constraints(const DevModel* m, EnvLDS& L) {
  int lane = wave_lane();
  // ---- scalar rows: frictionloss (dof order) then active joint limits (joint order).  Lane d < 6 proposes dof d's
  // frictionloss row, lane 8 + 2 h + side the limit row of joint h; the active ones are compacted in lane order, which is
  // the list order above.  (One lane used to build the list in a loop: six impedance / solref evaluations in series.)
  {
    bool active = false;
    Row1 r; r.dof = 0; r.sign = 0.f; r.R = 1.f; r.aref = 0.f; r.floss = 0.f; r.f = 0.f; r.Ainv = 0.f; r.pad = 0.f;
    if (lane < NARM) {
      int d = lane;
      if (m->frictionloss[d] > 0.f) {
        float imp = impedance(m->dof_solimp, 0.f), K, B;
        kb_from_solref(m, m->dof_solref, m->dof_solimp, &K, &B);
        r.dof = d; r.sign = 1.f; r.floss = m->frictionloss[d];
        r.R = fmaxf(MINVAL_F, (1.f - imp) * m->dof_invweight0[d] / imp);
        r.aref = -B * L.qvel[d];
        r.f = 0.f; r.Ainv = 1.f / (L.Minv[d][d] + r.R);
        active = true;
      }
    } else if (lane >= 8 && lane < 8 + 2 * NARM) {
      int h = (lane - 8) >> 1, side = (lane - 8) & 1;
      if (m->limited[h]) {
        float q = L.qpos[h];
        float pos = side == 0 ? q - m->range[h][0] : m->range[h][1] - q;
        if (pos < 0.f) {
          float imp = impedance(m->jnt_solimp, pos), K, B;
          kb_from_solref(m, m->jnt_solref, m->jnt_solimp, &K, &B);
          r.dof = h; r.sign = side == 0 ? 1.f : -1.f; r.floss = 0.f;
          r.R = fmaxf(MINVAL_F, (1.f - imp) * m->dof_invweight0[h] / imp);
          r.aref = -B * r.sign * L.qvel[h] - K * imp * pos;
          r.f = 0.f; r.Ainv = 1.f / (L.Minv[h][h] + r.R);
          active = true;
        }
      }
    }
    unsigned long long mask = wave_ballot(active);
    if (active) L.row[wave_prefix(mask)] = r;
    // arm-pool slots for contacts that touch an arm link (in contact order): lane = contact
    bool arm = false;
    if (lane < L.ncon) { const Contact& c = L.con[lane]; arm = (c.d1 >= 0 && c.d1 < NARM) || (c.d2 >= 0 && c.d2 < NARM); }
    unsigned long long amask = wave_ballot(arm);
    if (arm) {
      int slot = wave_prefix(amask);
      // slots beyond the LDS pool keep their number: such a contact's Jacobian is not parked in the pool but computed again by the lane
      // that owns the contact when the Newton solver loads it (conreg_load: the same lane, the same expressions, the same bits), so NO arm
      // contact is ever dropped (round 5; until round 4 the tail of the pool was cut off and counted).  The PGS kernels stop at 32 contacts
      // and never get here.
      L.con[lane].armslot = slot;
    }
    int narm = __popcll(amask);
    if (lane == 0) {
      L.nrow = __popcll(mask);
      L.narmcon = narm < MAXARMCON ? narm : MAXARMCON;
    }
  }
  wave_sync();
  // ---- contact rows: lane = contact
  int ncon = L.ncon;
  if (lane < ncon) {
    Contact& c = L.con[lane];
    float solref[2] = {c.aref[0], c.aref[1]}, solimp[5] = {c.f[0], c.f[1], c.f[2], c.f[3], c.f[4]};
    float imp = impedance(solimp, c.dist), K, B;
    kb_from_solref(m, solref, solimp, &K, &B);
    float tran = 0.f;      // body_invweight0 of a free prop scales with 1 / mass scale
    if (c.d1 >= 0) tran += m->dyn_invweight0[c.d1][0] / (c.d1 >= NARM ? L.fscale[c.d1 - NARM] : 1.f);
    if (c.d2 >= 0) tran += m->dyn_invweight0[c.d2][0] / (c.d2 >= NARM ? L.fscale[c.d2 - NARM] : 1.f);
    float R0 = fmaxf(MINVAL_F, (1.f - imp) * tran / imp);
    float R1 = R0 / fmaxf(MINVAL_F, m->impratio);
    float mu0 = c.fric[0];
    c.R[0] = R0; c.R[1] = R1;
    c.R[2] = fmaxf(MINVAL_F, R1 * mu0 * mu0 / (c.fric[1] * c.fric[1]));
    c.R[3] = fmaxf(MINVAL_F, R1 * mu0 * mu0 / (c.fric[2] * c.fric[2]));
    c.mu = mu0 * sqrtf(R1 / R0);
    // row velocities J qvel: translational rows j<3 use frame[j] at the contact point, rotational rows frame[j-3]
    float vel[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int side = 0; side < 2; side++) {
      int d = side == 0 ? c.d1 : c.d2;
      float sgn = side == 0 ? -1.f : 1.f;
      if (d >= NARM) {
        int f = d - NARM;
        float r[3] = {c.pos[0] - L.xipos[d][0], c.pos[1] - L.xipos[d][1], c.pos[2] - L.xipos[d][2]};
        float wr[3]; cross3(wr, &L.fvel[f][3], r);
        float pv[3] = {L.fvel[f][0] + wr[0], L.fvel[f][1] + wr[1], L.fvel[f][2] + wr[2]};      // velocity of the contact point
#pragma unroll
        for (int j = 0; j < 3; j++) { vel[j] += sgn * dot3(&c.frame[3 * j], pv); vel[3 + j] += sgn * dot3(&c.frame[3 * j], &L.fvel[f][3]); }
      }
    }
    if (c.armslot >= 0) {
      // Arm part, ONCE per contact: J = J(link of geom2) - J(link of geom1) in the 6 arm dofs (either side may
      // be static or a free body; for arm-arm self-collision both contribute), kept dof-major in this contact's
      // slot of the LDS pool.
      const bool pooled = c.armslot < MAXARMCON;
      ArmCon& ac = L.armcon[pooled ? c.armslot : 0];
#pragma unroll
      for (int j = 0; j < 6; j++) {
        float Jd[NARM];
        arm_contact_row(L, c, j, Jd);
        float vj = 0.f;
#pragma unroll
        for (int q = 0; q < NARM; q++) { if (pooled) ac.Jt[q][j] = Jd[q]; vj += Jd[q] * L.qvel[q]; }
        vel[j] += vj;
      }
    }
#pragma unroll
    for (int j = 0; j < 6; j++) {
      c.aref[j] = -B * vel[j] - (j == 0 ? K * imp * c.dist : 0.f);
      c.f[j] = 0.f;
    }
  }
  wave_sync();
}

#include "so101_solver.hpp"
#include "so101_newton.hpp"

// ------------------------------------------------------------------ forward + Euler
// `phases` is a profiling aid of so101_physics (StepParams.phases, 7 = everything): bit0 collision, bit1 constraint
// rows + solve, bit2 solve iterations.
DEV void forward_smooth(const DevModel* m, EnvLDS& L) {
  kinematics(m, L);
  crba_arm(m, L);
  smooth_dynamics(m, L);
}

// solver coordinates -> MuJoCo's generalized accelerations
DEV void forward_accelerations(EnvLDS& L) {
  int lane = wave_lane();
  if (lane < NARM) L.qacc[lane] = L.qacc_arm[lane];
  if (lane >= 32 && lane < 32 + NFREE) {
    int f = lane - 32, b = NARM + f;
    float r[3] = {L.xipos[b][0] - L.xpos[b][0], L.xipos[b][1] - L.xpos[b][1], L.xipos[b][2] - L.xpos[b][2]};
    float al[3] = {L.facc[f][3], L.facc[f][4], L.facc[f][5]}, ww[3] = {L.fvel[f][3], L.fvel[f][4], L.fvel[f][5]};
    float t1[3], t2[3], ab[3];
    cross3(t1, al, r); cross3(t2, ww, r); cross3(t2, ww, t2);
    matTvec3(ab, L.xmat[b], al);
#pragma unroll
    for (int i = 0; i < 3; i++) { L.qacc[NARM + 6 * f + i] = L.facc[f][i] - t1[i]; L.qacc[NARM + 6 * f + 3 + i] = ab[i]; }
  }
  wave_sync();
}


// constraint rows + solve for the contacts in L.con, then back to MuJoCo's generalized accelerations.
// SOLVER is a compile-time choice (SO101_SOLVER_NEWTON / SO101_SOLVER_PGS): every kernel exists once per solver, so
// the Newton kernels carry no PGS code (and no PGS-only constraint data) and vice versa.
template <int SOLVER>
DEV void forward_constrained(const DevModel* m, EnvLDS& L, int max_iter, float tolerance, int phases) {
  if (phases & 2) {
    make_constraints(m, L);
    if constexpr (SOLVER == 1) solve_newton(m, L, (phases & 4) ? max_iter : 0, tolerance);
    else solve_pgs(m, L, (phases & 4) ? max_iter : 0, tolerance);
  }
  forward_accelerations(L);
}

template <int SOLVER>
DEV void forward(const DevModel* m, EnvLDS& L, int max_iter, float tolerance, int phases = 7) {
  forward_smooth(m, L);
  unsigned long long t0 = SO101_CLOCK();
  if (phases & 1) collision(m, L);
  else { if (wave_lane() == 0) { L.ncand = 0; L.ncon = 0; L.narmcon = 0; } wave_sync(); }
  unsigned long long t1 = SO101_CLOCK();
  forward_constrained<SOLVER>(m, L, max_iter, tolerance, phases);
  if (SO101_CLOCKS_ON && wave_lane() == 0) { L.t_collision += (unsigned int)(t1 - t0); L.t_solve += (unsigned int)(SO101_CLOCK() - t1); }
}

DEV void euler(const DevModel* m, EnvLDS& L) {
  int lane = wave_lane();
  float dt = m->dt;
  if (lane < NV) { L.qvel[lane] += dt * L.qacc[lane]; L.warm[lane] = L.qacc[lane]; }
  wave_sync();
  if (lane < NARM) L.qpos[lane] += dt * L.qvel[lane];
  if (lane >= 32 && lane < 32 + NFREE) {
    int f = lane - 32;
    float* q = &L.qpos[NARM + 7 * f]; const float* v = &L.qvel[NARM + 6 * f];
    q[0] += dt * v[0]; q[1] += dt * v[1]; q[2] += dt * v[2];
    float w[3] = {v[3], v[4], v[5]};
    float ang = dt * normalize3(w);
    float sn, cs; sincos_f(0.5f * ang, &sn, &cs);
    float dq[4] = {cs, w[0] * sn, w[1] * sn, w[2] * sn};
    float qq[4] = {q[3], q[4], q[5], q[6]};
    mulquat(qq, qq, dq);
    normquat(qq);
    q[3] = qq[0]; q[4] = qq[1]; q[5] = qq[2]; q[6] = qq[3];
  }
  wave_sync();
}

// mj_checkPos / mj_checkVel / mj_checkAcc: a NaN or |x| > 1e10 anywhere in the state means the simulation
// diverged; MuJoCo resets the data to qpos0, dm_control (raise_exception_on_physics_error=False,
// so101_sim/task_suite.py:153) ends the episode with reward 0 and discount 0.  Returns true when diverged.
DEV bool check_divergence(EnvLDS& L) {
  int lane = wave_lane();
  bool bad = false;
  if (lane < NQ) { float x = L.qpos[lane]; bad = bad || !(fabsf(x) <= 1e10f); }
  if (lane < NV) { float x = L.qvel[lane], y = L.qacc[lane]; bad = bad || !(fabsf(x) <= 1e10f) || !(fabsf(y) <= 1e10f); }
  bool any = wave_ballot(bad) != 0ull;
  if (any) {
    wave_sync();
    if (lane < NQ) L.qpos[lane] = (lane == NARM + 3 || lane == NARM + 10) ? 1.f : 0.f;
    if (lane < NV) { L.qvel[lane] = 0.f; L.warm[lane] = 0.f; L.qacc[lane] = 0.f; }
    if (lane == 0) L.overflow |= 8;
    wave_sync();
  }
  return any;
}

template <int SOLVER>
DEV bool substep(const DevModel* m, EnvLDS& L, int max_iter, float tolerance, bool freeze_arm, int phases = 7) {
  forward<SOLVER>(m, L, max_iter, tolerance, phases);
  euler(m, L);
  if (check_divergence(L)) return true;
  if (freeze_arm) {   // dm_control JointStaticIsolator: non-prop joints restored after every step
    int lane = wave_lane();
    if (lane < NARM) { L.qpos[lane] = L.arm0_q[lane]; L.qvel[lane] = L.arm0_v[lane]; }
    wave_sync();
  }
  return false;
}

// ------------------------------------------------------------------ reward (uniform): so100_hand_over.py:238-275
// requires kinematics() of the current qpos to be in LDS
DEV float task_reward(const DevModel* m, const EnvLDS& L) {
  // any_props_moving: linear part only, >= 1e-3 (success_detector_utils.py:22-28)
#pragma unroll
  for (int f = 0; f < NFREE; f++) {
    const float* v = &L.qvel[NARM + 6 * f];
    float mx = fmaxf(fabsf(v[0]), fmaxf(fabsf(v[1]), fabsf(v[2])));
    if (mx >= 1e-3f) return 0.f;
  }
  int ob = NARM + 0, cb = NARM + 1;
  BoxW o;
  float im[9], xim[9];
  quat2mat(im, m->free_iquat[0]);
  matmul3(xim, L.xmat[ob], im);
  mat2quat(o.quat, xim);
  float ctr[3]; rotvecquat(ctr, m->free_bvh[0], o.quat);
#pragma unroll
  for (int i = 0; i < 3; i++) { o.pos[i] = ctr[i] + L.xipos[ob][i]; o.half[i] = m->free_bvh[0][3 + i]; }
  const float* cq_ = &L.qpos[NARM + 7 + 3];
  float cq[4] = {cq_[0], cq_[1], cq_[2], cq_[3]};
  normquat(cq);
  for (int k = 0; k < m->nbox; k++) {
    BoxW cw;
    float r[3]; rotvecquat(r, m->box_pos[k], cq);
#pragma unroll
    for (int i = 0; i < 3; i++) { cw.pos[i] = L.xpos[cb][i] + r[i]; cw.half[i] = m->box_half[k][i]; }
    float ident[4] = {1.f, 0.f, 0.f, 0.f};
    mulquat(cw.quat, cq, ident);
    if (!overlap_oobb_oobb(o, cw)) return 0.f;
  }
  return 1.f;
}
