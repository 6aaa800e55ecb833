// Translation unit: PGS instantiations of so101_physics, so101_debug_forward and so101_contacts.
#include "so101_kernels.hpp"
#include "so101_contacts.hpp"
#include "so101_launch.hpp"

namespace so101 {
void launch_physics_pgs(int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, int nsub, int freeze, int* diag) {
  hipLaunchKernelGGL(k_physics<0>, dim3(n_envs), dim3(64), 0, st, m, P, B, nsub, freeze, diag);
}
void launch_debug_forward_pgs(int n_envs, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, float* out) {
  hipLaunchKernelGGL(k_debug_forward<0>, dim3(n_envs), dim3(64), 0, st, m, P, B, out);
}
void launch_contacts_pgs(int n, hipStream_t st, const DevModel* m, const StepParams& P, const DevBuffers& B, const int* env_index, int forces,
                         const TouchPairsT<4>& T, const ContactOut& O) {
  hipLaunchKernelGGL(k_contacts<0>, dim3((unsigned int)n), dim3(64), 0, st, m, P, B, env_index, forces, T, O);
}
}  // namespace so101
