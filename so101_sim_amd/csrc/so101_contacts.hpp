// Contact sensing (so101_contacts of include/so101.h): the contact list of an env's CURRENT bound state and its reduction over pairs of geom
// groups, one wavefront per reported env.  The pass is MuJoCo's mj_forward cut down to what the report needs: load_state, kinematics and
// collision for the geometry; with `forces` also crba_arm, smooth_dynamics, make_constraints and the configured solver, with the iterations,
// tolerance and warmstart k_debug_forward uses.  Nothing is stored back - no bound buffer changes, the warmstart included.
//
// Where the numbers come from (read in the code, and checked bit for bit against the stage dump by the tests):
//   * Contact::frame is the FULL frame: contact_init() (so101_device.hpp) puts the normal (geom1 -> geom2) into row 0 and make_frame()
//     completes rows 1 and 2, MuJoCo's contact.frame.  The stage dump only shows row 0.
//   * Contact::f after the solve is the contact's force in that frame, what mj_contactForce returns and what DBG_FORCE dumps: solve_newton()
//     and solve_pgs() write all six entries on leaving, the ones beyond the contact's dim as zeros.  Before the solve the field holds the
//     mixed solimp (contact_init) - which is why `force` and the force sums need forces != 0 and are never written without it.
//   * L.overflow after the pass is diag word 4 of THIS pass: 1 candidate overflow, 2 contact overflow, 128 reduced to one contact per pair
//     from collision(); with forces the solve's bits as well (PGS: 2 when it drops the contacts beyond its 32).
//
// Everything after the pass - the stores in the ABI's order and the reduction over the group pairs - is contact_report() of
// so101_contact_report.hpp, shared with the general-tree engine; MAXCON is 64, one lane per contact and one pass.
#pragma once
#include "so101_env.hpp"
#include "so101_contact_report.hpp"

// what contact_report() reads of this engine: the list and the flag word in EnvLDS, the force where the solvers leave it
struct EnvContactView {
  static constexpr int DIST = (int)(offsetof(Contact, dist) / 4), POS = (int)(offsetof(Contact, pos) / 4), FRAME = (int)(offsetof(Contact, frame) / 4);
  const EnvLDS& L;
  int count, flags;
  DEV int g1(int k) const { return L.con[k].g1; }
  DEV int g2(int k) const { return L.con[k].g2; }
  DEV const float* words(int k) const { return (const float*)&L.con[k]; }
  DEV float force(int k, int j) const { return L.con[k].f[j]; }
};

template <int SOLVER>
__global__ void __launch_bounds__(64) k_contacts(const DevModel* m, StepParams P, DevBuffers B, const int* env_index, int forces, TouchPairsT<4> T, ContactOut O) {
  __shared__ EnvLDS L;
  const size_t i = blockIdx.x;
  const int e = env_index ? wave_uniform_i(env_index[i]) : (int)i;
  if (e < 0 || e >= P.n_envs) { contacts_outside<MAXCON>(i, T.npair, O); return; }
  load_state(L, B, e, P.n_envs);
  kinematics(m, L);
  if (forces) {                     // (wave-uniform: a kernel argument)
    crba_arm(m, L);
    smooth_dynamics(m, L);
  }
  collision(m, L);
  if (forces) {
    make_constraints(m, L);
    if constexpr (SOLVER == 1) solve_newton(m, L, P.iterations, P.tolerance); else solve_pgs(m, L, P.iterations, P.tolerance);
  }
  wave_sync();
  contact_report<MAXCON>(i, EnvContactView{L, L.ncon, L.overflow}, forces != 0, T, O);
}
