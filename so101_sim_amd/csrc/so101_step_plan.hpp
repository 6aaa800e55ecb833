// Launch plans of the control step of both engines, as data: how many launch chains run, where the envs are cut into slices, how many
// persistent narrowphase wavefronts a slice gets, which k_narrow instance runs and how many pairs a work item fetch takes.  The step functions
// (enqueue_pipelined of so101_hip.hip, so101_tree_step of tu_tree.hip) execute a plan and decide nothing themselves; tests/test_step_plan.py
// holds the plans of the sizes that matter as literal tables.
// Plain C++17: no HIP header, everything inline, outside every namespace, no T* macro (the tree engine is compiled twice, the emulator build of
// the tests puts every .hip into one translation unit).  plan_so100_step() and plan_tree_step() are pure: same arguments, same plan.
// Every threshold below was measured; the numbers are in profiles/README.md, "Launch-plan thresholds: what was measured".
#pragma once
#include <cstdlib>

#ifndef NARROW_CHUNK
#define NARROW_CHUNK 4     // candidate pairs per narrowphase work item
#endif
#ifndef SO101_LIST_ROWS_DEFAULT
#define SO101_LIST_ROWS_DEFAULT 1     // k_narrow<false>'s list row pass where SO101_NARROW_LIST_ROWS is unset (profiles/README.md, "Launch-plan thresholds")
#endif

constexpr int STEP_PLAN_MAX_SLICES = 8;      // launch chains of a step at most (so101_sim::MAXGROUPS; TreeHandle::MAXSLICES is below it)

// Experiment overrides (tests and kernel experiments), read from the environment by read_step_knobs() every time a step is enqueued - with
// graph replay: at every capture -, so a handle configured after a change sees it.  0 / -1 / NULL: not set, the plan's own rule holds.
struct StepKnobs {
  int narrow_chunk = 0;              // SO101_NARROW_CHUNK: heavy pairs per fetch, 1 .. NARROW_CHUNK
  int narrow_chunk_light = 0;        // SO101_NARROW_CHUNK_LIGHT: light pairs per fetch, 1 .. NARROW_CHUNK
  int narrow_rows = -1;              // SO101_NARROW_ROWS: 0 / 1 = k_narrow<true>'s row pass off / on
  int narrow_list_rows = -1;         // SO101_NARROW_LIST_ROWS: 0 / 1 = k_narrow<false>'s list row pass off / on (the row pass wins over it)
  int narrow_waves_q = 0;            // SO101_NARROW_WAVES_Q: quarter narrowphase wavefronts per env
  int tree_slices = 0;               // SO101_TREE_SLICES: env slices of the tree engine's chain, 1 .. max_slices
  int tree_narrow_waves_q = 0;       // SO101_TREE_NARROW_WAVES_Q: quarter narrowphase wavefronts per env, tree engine
  const char* debug_bounds = nullptr;      // SO101_DEBUG_BOUNDS ("128,1024" = slice ends), read in SO101_DEBUG_CLOCKS builds only
};

inline StepKnobs read_step_knobs() {
  auto num = [](const char* name, int unset) { const char* v = getenv(name); return v ? atoi(v) : unset; };
  StepKnobs K;
  K.narrow_chunk = num("SO101_NARROW_CHUNK", 0); K.narrow_chunk_light = num("SO101_NARROW_CHUNK_LIGHT", 0);
  K.narrow_rows = num("SO101_NARROW_ROWS", -1); K.narrow_list_rows = num("SO101_NARROW_LIST_ROWS", -1);
  K.narrow_waves_q = num("SO101_NARROW_WAVES_Q", 0);
  K.tree_slices = num("SO101_TREE_SLICES", 0); K.tree_narrow_waves_q = num("SO101_TREE_NARROW_WAVES_Q", 0);
#ifdef SO101_DEBUG_CLOCKS
  K.debug_bounds = getenv("SO101_DEBUG_BOUNDS");
#endif
  return K;
}

// Hardware queues the HIP runtime maps this process' streams onto: GPU_MAX_HW_QUEUES (its default 4), or SO101_HW_QUEUES_EFFECTIVE where a
// host knows that variable came too late for the runtime (so101_sim_amd/__init__.py).  Read ONCE per process: the runtime honours the variable
// only before it initialises, a later value would misreport the queues.
inline int hw_queues() {
  static const int q = getenv("SO101_HW_QUEUES_EFFECTIVE") ? atoi(getenv("SO101_HW_QUEUES_EFFECTIVE")) : (getenv("GPU_MAX_HW_QUEUES") ? atoi(getenv("GPU_MAX_HW_QUEUES")) : 4);
  return q;
}
constexpr int STEP_PLAN_QUEUES_FOR_FOUR_CHAINS = 6;      // the step uses chains + 2 streams, and streams that share a queue serialise

// ---- SO100 engine: the launch chains of so101_step (pipeline 1, and the slices of pipeline 3)
struct StepPlan {
  int G = 1;                                   // launch chains = slices of the cost-sorted env order (most expensive first)
  int bounds[STEP_PLAN_MAX_SLICES + 1] = {};   // slice g holds sorted positions bounds[g] .. bounds[g + 1]
  int deal = 1;                                // k_order's argument: G = the sorted envs are dealt out over G equal slices, 1 = plain sorted order
  bool rows = false, list_rows = false;        // k_narrow<true>'s row pass / k_narrow<false>'s list row pass
  unsigned int narrow_chunk = 0;               // PipeBuffers::narrow_chunk: heavy pairs per fetch | light pairs << 4 | rows << 8 | list_rows << 9
  int waves[STEP_PLAN_MAX_SLICES] = {};        // persistent narrowphase wavefronts of slice g
};

inline StepPlan plan_so100_step(int n_envs, int cfg_groups, int hw_queues, const StepKnobs& K) {
  StepPlan P;
  const int n = n_envs;
  // chains: four where the runtime has the queues for them, else three (four on four queues: 400 k against 650 k env-steps/s); a batch below
  // 64 envs is one chain of dependent launches whatever is asked for
  int G = cfg_groups > 0 ? cfg_groups : (hw_queues >= STEP_PLAN_QUEUES_FOR_FOUR_CHAINS ? 4 : 3);
  if (G > STEP_PLAN_MAX_SLICES) G = STEP_PLAN_MAX_SLICES;
  if (n < 64) G = 1;
  // slices: 2 chains split at n/2, 3 at n/4 and 5n/8 (the first slice holds the expensive envs), 4 and more in equal parts (unequal 4-way
  // splits are 1-2 % slower)
  int* b = P.bounds;
  b[0] = 0;
  if (G == 2) b[1] = n / 2;
  if (G == 3) { b[1] = n / 4; b[2] = (5 * n) / 8; }
  if (G > 3) for (int g = 1; g < G; g++) b[g] = (int)((long long)n * g / G);
  b[G] = n;
  if (K.debug_bounds) {      // profiling builds: the ascending values below n are the slice ends
    G = 0;
    for (const char* p = K.debug_bounds; *p && G < STEP_PLAN_MAX_SLICES - 1;) { int v = atoi(p); if (v > b[G] && v < n) b[++G] = v; while (*p && *p != ',') p++; if (*p) p++; }
    b[++G] = n;
  }
  P.G = G;
  // equal slices get the sorted envs dealt out (every chain the same mix of expensive and cheap envs); unequal ones keep the plain sorted order
  bool equal_slices = G > 1;
  for (int g = 0; g < G && equal_slices; g++) equal_slices = b[g + 1] - b[g] == n / G;
  P.deal = equal_slices && n % G == 0 ? G : 1;
  // the row pass pays above 8192 envs only (at 4096 the step follows its slowest slice, not the light pairs' instruction count)
  P.rows = K.narrow_rows >= 0 ? K.narrow_rows != 0 : n > 8192;
  // the list row pass pays above 2048 envs (2048: 491 k -> 455 k env-steps/s with it)
  P.list_rows = !P.rows && (K.narrow_list_rows >= 0 ? K.narrow_list_rows != 0 : (SO101_LIST_ROWS_DEFAULT && n > 2048));
  // heavy pairs per fetch: 1 up to 4096 envs - 2 where the list row pass runs by default: the launch then ends on its heavy pairs -, 2 up to 8192, 4 above
  const int ch = K.narrow_chunk >= 1 && K.narrow_chunk <= NARROW_CHUNK ? K.narrow_chunk : (n <= 4096 ? (P.list_rows && n > 2048 ? 2 : 1) : (n <= 8192 ? 2 : NARROW_CHUNK));
  // light pairs per fetch: 4 under the list row pass (its items stage no hull, so four cannot overflow the LDS pool), else 1 for a handful of
  // envs (their few pairs spread over the wavefronts), 2 up to 8192 envs, 4 above
  const int cl = K.narrow_chunk_light >= 1 && K.narrow_chunk_light <= NARROW_CHUNK ? K.narrow_chunk_light
                 : (P.list_rows ? NARROW_CHUNK : (n <= 16 ? 1 : (n <= 8192 ? 2 : NARROW_CHUNK)));
  P.narrow_chunk = (unsigned int)ch | ((unsigned int)cl << 4) | (P.rows ? 256u : 0u) | (P.list_rows ? 512u : 0u);
  // persistent narrowphase wavefronts (they pull work items until the list is empty): 1.25 per env of the slice up to 4096 envs, 1.5 up to 8192,
  // 2 above; at least 16 (a handful of envs is a chain of dependent launches: an env's pairs spread over 16 wavefronts), at most what fills 256
  // CUs - a smaller narrowphase grid leaves slots to the other chains' solve kernels
  const int nw_quarters = K.narrow_waves_q > 0 ? K.narrow_waves_q : (n <= 4096 ? 5 : (n <= 8192 ? 6 : 8));
  for (int g = 0; g < G; g++) {
    const int nw = (int)((long long)(b[g + 1] - b[g]) * nw_quarters / 4);
    P.waves[g] = nw < 16 ? 16 : (nw < 4096 ? nw : 4096);
  }
  return P;
}

// ---- general-tree engine: so101_tree_step
struct TreeStepPlan {
  bool chain = false;            // the launch chain (prologue, then per substep narrowphase and solve); false: the single kernel k_tree_step
  int G = 1;                     // env slices, each on its own stream (the single kernel: one, the whole batch)
  struct Slice { int e0, ng, nw; } slice[STEP_PLAN_MAX_SLICES] = {};      // first env, envs, narrowphase wavefronts (0: single kernel)
};

// post: contact rewards end the chain with one more narrowphase launch on the post-step state, which takes a work-list slot like a substep
// (max_sub of them); chain_ready: the handle was configured for the chain and has its buffers
inline TreeStepPlan plan_tree_step(int n_envs, int n_substeps, bool post, bool chain_ready, int max_slices, int max_sub, const StepKnobs& K) {
  TreeStepPlan P;
  P.chain = chain_ready && n_substeps + (post ? 1 : 0) <= max_sub;
  if (!P.chain) { P.slice[0] = {0, n_envs, 0}; return P; }
  if (max_slices > STEP_PLAN_MAX_SLICES) max_slices = STEP_PLAN_MAX_SLICES;
  // slices: the narrowphase of one runs beside the solve of another; 2 from 128 envs, 4 from 512 (ALOHA 4096 envs, 1 / 2 / 4 slices: 206 / 232 / 231 k)
  P.G = n_envs < 128 ? 1 : (K.tree_slices >= 1 && K.tree_slices <= max_slices ? K.tree_slices : (n_envs < 512 ? 2 : 4));
  for (int g = 0; g < P.G; g++) {
    const int e0 = (int)((long long)n_envs * g / P.G), ng = (int)((long long)n_envs * (g + 1) / P.G) - e0;
    // two narrowphase wavefronts per env of the slice, at most what fills 256 CUs
    const int nw = (int)((long long)ng * (K.tree_narrow_waves_q > 0 ? K.tree_narrow_waves_q : 8) / 4);
    P.slice[g] = {e0, ng, nw < 1 ? 1 : (nw < 4096 ? nw : 4096)};
  }
  return P;
}
