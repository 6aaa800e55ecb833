// TEST HARNESS ONLY: the two launch-plan functions of so101_sim_amd/csrc/so101_step_plan.hpp behind a C interface (tests/test_step_plan.py).
// Host compiler only: the header includes nothing of HIP.
#include "so101_step_plan.hpp"

namespace {
// knobs[7]: narrow_chunk, narrow_chunk_light, narrow_rows, narrow_list_rows, narrow_waves_q, tree_slices, tree_narrow_waves_q (StepKnobs order)
StepKnobs knobs_of(const int* k) {
  StepKnobs K;
  K.narrow_chunk = k[0]; K.narrow_chunk_light = k[1]; K.narrow_rows = k[2]; K.narrow_list_rows = k[3]; K.narrow_waves_q = k[4];
  K.tree_slices = k[5]; K.tree_narrow_waves_q = k[6];
  return K;
}
}  // namespace

extern "C" {

int plan_probe_max_slices(void) { return STEP_PLAN_MAX_SLICES; }

// the knobs as read_step_knobs() finds them in the environment, in the order of knobs_of()
void plan_probe_read_knobs(int* out) {
  const StepKnobs K = read_step_knobs();
  const int v[7] = {K.narrow_chunk, K.narrow_chunk_light, K.narrow_rows, K.narrow_list_rows, K.narrow_waves_q, K.tree_slices, K.tree_narrow_waves_q};
  for (int i = 0; i < 7; i++) out[i] = v[i];
}

// head[6] = G, deal, rows, list_rows, narrow_chunk, 0; bounds[MAX + 1]; waves[MAX]
void plan_probe_so100(int n_envs, int cfg_groups, int hw_queues, const int* knobs, const char* debug_bounds, int* head, int* bounds, int* waves) {
  StepKnobs K = knobs_of(knobs);
  K.debug_bounds = debug_bounds;
  const StepPlan P = plan_so100_step(n_envs, cfg_groups, hw_queues, K);
  head[0] = P.G; head[1] = P.deal; head[2] = P.rows; head[3] = P.list_rows; head[4] = (int)P.narrow_chunk; head[5] = 0;
  for (int g = 0; g <= STEP_PLAN_MAX_SLICES; g++) bounds[g] = P.bounds[g];
  for (int g = 0; g < STEP_PLAN_MAX_SLICES; g++) waves[g] = P.waves[g];
}

// head[2] = chain, G; slices[MAX][3] = e0, ng, nw
void plan_probe_tree(int n_envs, int n_substeps, int post, int chain_ready, int max_slices, int max_sub, const int* knobs, int* head, int* slices) {
  const TreeStepPlan P = plan_tree_step(n_envs, n_substeps, post != 0, chain_ready != 0, max_slices, max_sub, knobs_of(knobs));
  head[0] = P.chain; head[1] = P.G;
  for (int g = 0; g < STEP_PLAN_MAX_SLICES; g++) { slices[3 * g] = P.slice[g].e0; slices[3 * g + 1] = P.slice[g].ng; slices[3 * g + 2] = P.slice[g].nw; }
}

}  // extern "C"
