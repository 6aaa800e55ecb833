/* so101.h — C ABI of libso101_hip.so: the MI355X (gfx950) batched step of the SO100/SO101
 * hand-over environments.
 *
 * The reference (tuul-ai/so101_sim) has no FFI for this path: its boundary is the Python API
 *   so101_sim/task_suite.py:103-155   create_task_env(...) -> dm_control composer.Environment
 *   env.reset() / env.step(action)    (dm_control loop; hooks in so101_sim/tasks/base/so100_task.py:266-320,
 *                                      so101_sim/tasks/so100_hand_over.py:238-323)
 * and all arithmetic happens inside mujoco.mj_step (third party).  Each entry point below names the
 * reference call it stands in for.  The Python shim so101_sim_amd/env.py binds these with ctypes
 * (INTEGRATION.md shows the binding a reference maintainer would add).
 *
 * Conventions
 *  - return 0 on success, negative so101_status otherwise; no C++ exception crosses the boundary;
 *    so101_last_error() gives a message for the last failing call on that handle (or on create).
 *  - every array argument is a DEVICE pointer owned by the caller (tensor.data_ptr()); the library
 *    never frees caller memory and keeps bound pointers until so101_destroy / the next bind.
 *  - state arrays are struct-of-arrays with the env index fastest: qpos[nq][N], qvel[nv][N], ...
 *    so that lanes reading one scalar for consecutive envs coalesce.
 *  - `hip_stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream); calls are
 *    asynchronous with respect to the host.
 *  - a handle is bound to one device (every entry point makes that device current for the duration of the call
 *    and restores the caller's) and is not thread-safe.
 *  - bound state buffers must stay allocated until so101_destroy or the next so101_bind_state returns: the reset
 *    prefetch reads them asynchronously on an internal stream (both calls drain it).
 */
#ifndef SO101_H_
#define SO101_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SO101_ABI_VERSION 10     /* 10: so101_tree_last_plan, and (additions that change nothing older, so the number stays) the cameras: so101_camera,
                                    so101_set_hull_planes, so101_render, so101_tree_set_hull_planes, so101_tree_render, the colour cameras: so101_shading, so101_color_out, so101_render_color, so101_tree_render_color, and Cartesian tool control: so101_tool, so101_ik_config, so101_ik_default_config,
                                    so101_tool_pose, so101_tool_ik, proximity sensing: so101_proximity_out, so101_proximity, so101_tree_proximity, and the same (tool control) for the general-tree engine: so101_tree_tool, so101_tree_ik_config, so101_tree_tool_chain,
                                    so101_tree_ik_default_config, so101_tree_tool_pose, so101_tree_tool_ik; 9: so101_tree_config gains the observation delays, so101_tree_bind_physics_state; 8: the general-tree engine (so101_tree_*) */
#define SO101_OBS_DIM 18      /* joints_pos(6, delayed) | undelayed_joints_pos(6) | commanded_joints_pos(6) */
#define SO101_ACT_DIM 6
#define SO101_SOLVER_PGS 0
#define SO101_SOLVER_NEWTON 1
#define SO101_RING_DEPTH 5    /* joints_pos delay: 0.1 s = 5 control steps (so100_task.py:81,196-198) */

typedef enum {
  SO101_OK = 0,
  SO101_ERR_ARG = -1,        /* NULL/invalid argument */
  SO101_ERR_MODEL = -2,      /* blob rejected (magic/version/dims outside the compiled limits) */
  SO101_ERR_HIP = -3,        /* HIP runtime error (message holds hipGetErrorString) */
  SO101_ERR_STATE = -4       /* call order violated (e.g. step before bind_state) */
} so101_status;

typedef struct so101_sim so101_sim; /* opaque */

/* Caller-owned device buffers holding the per-env state (struct-of-arrays, N fastest). */
typedef struct {
  float* qpos;         /* [nq][N]  generalized positions          (physics.data.qpos) */
  float* qvel;         /* [nv][N]  generalized velocities         (physics.data.qvel) */
  float* ctrl;         /* [nu][N]  actuator controls, UNclamped   (physics.data.ctrl) */
  float* warmstart;    /* [nv][N]  previous qacc (solver warm start, data.qacc_warmstart) */
  float* obs_ring;     /* [SO101_RING_DEPTH][6][N] joints_pos delay line */
  float* ep_return;    /* [N] running sum of rewards of the current episode */
  int32_t* step_count; /* [N] control steps since reset */
  int32_t* episode;    /* [N] episode counter (keys the reset RNG) */
  const float* mass_scale; /* [2][N] per-env scale of the free props' mass and inertia (object, container): domain
                          randomisation beyond the reference, which randomises poses only (so100_hand_over.py:37-55);
                          NULL = 1.0 everywhere.  Read at every step and reset; after changing values call
                          so101_configure (cached initial states were settled with the old masses). */
} so101_buffers;

/* Tunables that the reference fixes through its MJCF / dm_control arguments. */
typedef struct {
  float action_offset[SO101_ACT_DIM]; /* calibration homing offsets added to every action
                                         (scripts/so101_calibration.py:62-88; zeros when the file is absent) */
  int32_t last_step;       /* control step on which physics.time() >= time_limit first holds
                              (task_suite.py:151; fp64 accumulation replayed on the host) */
  int32_t n_substeps;      /* control_timestep / physics timestep = 10 (task_suite.py:41) */
  int32_t solver_iterations; /* solver iteration cap; <=0 keeps the model's (100) */
  float solver_tolerance;  /* solver early-exit tolerance; <0 keeps the model's (1e-8) */
  int32_t settle_max_substeps; /* PropPlacer settle budget, 1000 = 2.0 s (so100_hand_over.py:222-229) */
  int32_t terminate_on_success; /* SO100Task terminate_episode (so100_task.py:120,297-302) */
  uint64_t env_id_base;    /* global index of env 0 of this handle (multi-GPU sharding) */
  int32_t solver;          /* SO101_SOLVER_NEWTON (default: the reference's scene sets no <option solver>, so MuJoCo's
                              default Newton applies) or SO101_SOLVER_PGS (the solver BASELINE.json's north_star names) */
  int32_t prefetch_resets; /* 1 (default): settle the next episode's initial state of every env ahead of time on an
                              internal low-priority stream, so that auto-resets inside so101_step cost a copy;
                              0: always settle inside the call.  Results are identical either way. */
  int32_t pipeline;        /* how so101_step is launched; same device functions, bit-identical results:
                              1 (default) launch chains: per env slice, every substep is a narrowphase launch (one
                                wavefront per candidate pair) followed by a solve launch (one wavefront per env);
                              0 one fused launch, one wavefront per env;
                              2 per-env chained: cost order, prologue and ONE persistent launch whose wavefronts pull
                                narrowphase chunks and per-env solve items from device-side queues, every env advancing
                                on its own dependencies (csrc/so101_chain.hpp);
                              3 merged launches: like 1, with the narrowphase of substep s + 1 pulled as chunks inside
                                the solve launch of substep s (half the launch boundaries).
                              2 and 3 are correct and measured slower on MI355X: wavefronts that run narrowphase and
                              solver code out of step refetch the 240 KB of code from L2 (profiles/README.md). */
  int32_t groups;          /* pipelined step: the envs, sorted by the solver time of their previous step, are cut into 1..8
                              slices whose launch chains run on separate internal streams and fill each other's tails;
                              0 (default) = 4 when GPU_MAX_HW_QUEUES >= 6 was set before HIP initialised, else 3 (the
                              runtime maps streams onto that many hardware queues; chains that share one serialise);
                              results do not depend on it */
  int32_t use_graph;       /* 1 (default): the launch sequence of the pipelined step is captured once into a HIP graph and
                              replayed with one hipGraphLaunch per step (re-captured when configuration, bound buffers,
                              pool or the step's I/O pointers change); 0: plain launches.  Same kernels either way. */
  int32_t chain_waves;     /* pipeline = 2: persistent wavefronts of the step kernel; 0 (default) = 2048 (2 per SIMD on
                              256 CUs), capped at 2 * N + 6 */
} so101_config;

int so101_version(void);

/* Compile-time limits of this build, for the host shim's sanity checks. */
int so101_max_contacts(void);

/* Replaces: composer.Environment construction + MuJoCo model compile (task_suite.py:148-155).
 * model_blob: f32 blob from so101_sim_amd/model/blob.py (host memory, copied).  Allocates the
 * device copy of the model and internal scratch only. */
int so101_create(const void* model_blob, size_t blob_bytes, int n_envs, int hip_device, uint64_t seed,
                 so101_sim** out);
void so101_destroy(so101_sim* sim);

int so101_default_config(so101_config* cfg);
int so101_configure(so101_sim* sim, const so101_config* cfg);
int so101_bind_state(so101_sim* sim, const so101_buffers* buffers);

/* Optional observables physics_state = concat(qpos, qvel) (shape (38,), so100_task.py:366-368; enabled by the reference iff
 * image_observation_enabled, :203) and delayed_physics_state, the same delayed by 0.3 s = 15 control steps and padded with the
 * episode's first value (:204-210, task_suite.py:154).  ring [15][38][N] is the delay line (caller-owned like obs_ring),
 * physics_state / delayed [N][38] are rewritten by every so101_step / so101_reset / so101_begin_episode.  All NULL = off
 * (default).  The pointers must stay valid like the bound state buffers. */
#define SO101_PHYSICS_STATE_DIM 38
#define SO101_PHYSICS_STATE_DELAY 15
int so101_bind_physics_state(so101_sim* sim, float* ring, float* physics_state, float* delayed_physics_state);

/* Replaces: env.reset() -> task.initialize_episode (so100_task.py:304-320, so100_hand_over.py:320-323):
 * arm qpos/qvel = 0, ctrl = home + offsets, object/container placement drawn from the counter RNG keyed
 * (seed, env_id, episode), container rejection-sampled against collisions, props settled with the arm
 * held, delay line filled with the reset value.  mask: [N] bytes, nonzero = reset that env; NULL = all. */
int so101_reset(so101_sim* sim, const uint8_t* mask, void* hip_stream);

/* Reset pool: with pool_size > 0 every reset (so101_reset and the auto-reset inside so101_step) starts the episode
 * from entry floor(u * pool_size) of the caller's pool, u = the counter RNG at (seed, global env id, episode, draw
 * 1000), instead of placement + settle: scripted pre-grasp states for contact-heavy workloads
 * (examples/automated_lerobot_dataset_generator.py:180-205 scripts such states on the reference), checkpoints.
 * qpos[20][K], qvel[18][K], ctrl[6][K] are device pointers that must outlive their use; pool_size = 0 restores the
 * reference's reset. */
int so101_set_reset_pool(so101_sim* sim, const float* qpos, const float* qvel, const float* ctrl, int pool_size);

/* Settled-state store: the 1000-substep PropPlacer settle of so100_hand_over.py:222-229 dominates short episodes, and its
 * result is a pure function of (model, seed, global env id, episode, mass scale, solver settings).
 * so101_compute_settled() runs placement + settle for episodes first_episode .. first_episode + n_episodes - 1 of
 * every env into caller-owned device tables qpos[n_episodes][20][N], qvel[..][18][N], warmstart[..][18][N],
 * flags[n_episodes][N] without touching the envs; the caller may keep them on disk across runs (the Python face
 * does: BatchedEnvironment.save_settled_cache / load_settled_cache).  so101_set_settled_store() hands such tables
 * back: resets of those episodes copy the entry (bit-identical to settling again) and the background prefetch skips
 * them.  n_episodes = 0 detaches the store.  The tables must outlive their use. */
int so101_compute_settled(so101_sim* sim, int first_episode, int n_episodes, float* qpos, float* qvel, float* warmstart,
                          int32_t* flags, void* hip_stream);
int so101_set_settled_store(so101_sim* sim, const float* qpos, const float* qvel, const float* warmstart,
                            const int32_t* flags, int first_episode, int n_episodes);

/* PropPlacer settle only (so100_hand_over.py:222-229, settle_physics=True): from the state in the bound buffers, arm
 * held, props integrated until |qvel| < 1e-3 and |qacc| < 1e-2 or settle_max_substeps are used.  For callers that draw
 * the placements themselves - the single-env Python facade draws them from numpy.random.RandomState in the reference's
 * order (object xyz, object yaw, container xyz per attempt), so that a seed reproduces the reference's episode; follow
 * with so101_begin_episode. */
int so101_settle(so101_sim* sim, void* hip_stream);

/* Starts an episode from whatever state the caller wrote into the bound buffers (checkpoint restore,
 * known-answer tests): ctrl = home + offsets, delay line filled with the current joints_pos,
 * step_count/ep_return cleared, no placement, no settle.  The reference's equivalent is
 * physics.set_state(...) followed by the observation updater's reset (dm_control). */
int so101_begin_episode(so101_sim* sim, void* hip_stream);

/* Replaces: env.step(action): before_step (so100_task.py:266-287), n_substeps x mj_step, observables
 * (so100_task.py:323-368 with the delays of :189-210), get_reward (so100_hand_over.py:238-275),
 * get_discount / termination (so100_task.py:292-302) and the time limit (task_suite.py:151).
 * Envs whose previous step was LAST are reset first and report FIRST (dm_control auto-reset).
 *   action    [N][6]  float32, row-major as the caller's (N,6) tensor
 *   obs       [N][SO101_OBS_DIM]
 *   reward    [N]  in {0,1}      discount [N] in {0,1}      step_type [N]: 0 FIRST, 1 MID, 2 LAST */
int so101_step(so101_sim* sim, const float* action, float* obs, float* reward, float* discount,
               uint8_t* step_type, void* hip_stream);

/* Physics only: n_substeps of mj_step on every env with the bound ctrl; no task logic.
 * freeze_arm != 0 restores the arm's qpos/qvel after every substep (PropPlacer settle). */
int so101_physics(so101_sim* sim, int n_substeps, int freeze_arm, void* hip_stream);

/* Reward of the current state (SO100HandOver.get_reward, overlap mode) -> reward[N]. */
int so101_reward(so101_sim* sim, float* reward, void* hip_stream);

/* Episode returns for logging (copied from the bound ep_return). */
int so101_get_returns(so101_sim* sim, float* out, void* hip_stream);

/* Diagnostics of the most recent substep, per env: [N][SO101_DIAG_DIM] int32
 *   0 ncon, 1 nefc, 2 solver iterations, 3 broadphase candidates, 4 overflow flags,
 *   5 collision time, 6 constraint+solver time, 7 whole-call time of this env's wavefront (10 ns ticks, summed over
 *   the substeps of the last call; words 5 and 7 are zero unless the library was built with -DSO101_DEBUG_CLOCKS). */
#define SO101_DIAG_DIM 8
int so101_get_diag(so101_sim* sim, int32_t* out, void* hip_stream);

/* Event counters since so101_create (or the last call with clear != 0): out is a DEVICE pointer to
 * SO101_NEVENTS uint64.  Counter b counts env-steps (b <= 3) or env-resets (b = 4, 5) on which flag b was raised:
 *   0 broadphase candidate list overflowed (candidates dropped)      1 contact list overflowed (contacts dropped)
 *   2 (retired in round 5, always 0: arm-link contacts beyond the LDS pool recompute their Jacobian instead of being dropped)
 *                                                                     3 physics diverged: NaN or |x| > 1e10 in the
 *     state (mj_checkPos/Vel/Acc); the episode ends with reward 0 / discount 0 like a dm_control PhysicsError
 *     (task_suite.py:153 raise_exception_on_physics_error=False)
 *   4 reset: the container placer's 20 attempts all collided (dm_control's PropPlacer raises RuntimeError there;
 *     here the last sample is kept and the event is counted)         5 reset: the settle did not converge within
 *     settle_max_substeps (dm_control warns, examples/so101_rl_breakdown.ipynb:50-55)
 *   6 chained steps (pipeline = 2) ended by the watchdog (scheduler protocol error).  The abort is sticky: that step's results and
 *     those of EVERY later chained step of the handle are invalid - each counts here - until so101_configure selects another step path
 *   7 more than so101_max_contacts() contacts in a substep: the env kept ONE contact per touching geom pair (the first of its patch) for
 *     that substep instead of cutting the list; counter 1 then only counts substeps whose touching PAIRS alone exceeded the limit
 * The same bits appear per env in diag word 4 for the most recent substep. */
#define SO101_NEVENTS 8
int so101_get_events(so101_sim* sim, uint64_t* out, int clear, void* hip_stream);

/* Stage dump of one forward pass (no integration) for parity tests against the oracle:
 * out is [N][SO101_DEBUG_DIM] float32; layout documented in csrc/so101_device.hpp (DBG_*). */
#define SO101_DEBUG_DIM 2048
int so101_debug_forward(so101_sim* sim, float* out, void* hip_stream);

/* Diagnostics of the pipelined step's last narrowphase launch (device buffers, any may be NULL):
 * ncand[N] (count | overflow << 16), cand[N][256] (geom1 | geom2 << 16), ticks[N][256] (10 ns per candidate; profiling builds
 * only, SO101_ERR_STATE otherwise), conres[48 N][24] (contact count, normal, 5 x (dist, position) per candidate, at the
 * candidates' work-list positions of the last substep - 48 records per env of a slice, mean use 12). */
/* (profiling builds, -DSO101_DEBUG_CLOCKS; zeros otherwise) Stage clocks of k_pipe_solve's second-to-last substep: stage[N][8] = smooth dynamics, contact gather, constraint
 * rows, solver, integrate, next broadphase (10 ns ticks), ncon, solver iterations. */
int so101_debug_stages(so101_sim* sim, uint32_t* stage, void* hip_stream);

int so101_debug_candidates(so101_sim* sim, int32_t* ncand, uint32_t* cand, uint32_t* ticks, float* conres, void* hip_stream);

/* Facts about the handle for logs and tests (host value, synchronises `hip_stream` for the device-side ones):
 *   SO101_INFO_GRAPH_ACTIVE   1 when the last so101_step replayed a captured HIP graph
 *   SO101_INFO_STEP_PATH      0 fused, 1 launch chains, 2 per-env chained: what the last so101_step ran
 *   SO101_INFO_CHAINS         launch chains of the last pipeline = 1 step
 *   SO101_INFO_HW_QUEUES      GPU_MAX_HW_QUEUES as the library read it (4 when unset)
 *   SO101_INFO_SCHED_ABORTS   times the chained step's watchdog ended a launch (a protocol error; also event 6)
 *   SO101_INFO_SCRATCH_BYTES  library-owned device memory of this handle
 *   SO101_INFO_NARROW_LIST_ROWS  1 when the last pipeline = 1 step enqueued the narrowphase with its list row pass (SO101_NARROW_LIST_ROWS) */
#define SO101_INFO_GRAPH_ACTIVE 0
#define SO101_INFO_STEP_PATH 1
#define SO101_INFO_CHAINS 2
#define SO101_INFO_HW_QUEUES 3
#define SO101_INFO_SCHED_ABORTS 4
#define SO101_INFO_SCRATCH_BYTES 5
#define SO101_INFO_NARROW_LIST_ROWS 6
long long so101_get_info(so101_sim* sim, int what, void* hip_stream);

/* Where the wavefronts of the chained step's persistent kernel spent their time since the last clear: out = 16 uint64 in
 * HOST memory (the call synchronises `hip_stream`): [0] claiming work that was found, [1] looking for work that was not,
 * [2] narrowphase chunks, [3] solve items (10 ns ticks, summed over wavefronts); [4] chunks, [5] solve items, [6] idle
 * rounds, [7] wavefronts that ran, [8] their lifetimes (ticks). */
int so101_debug_chain_stats(so101_sim* sim, uint64_t* out, int clear, void* hip_stream);

/* ---- depth and segmentation cameras: batched ray casting against the COLLISION geometry the step sees (csrc/so101_camera.hpp).  Stands in for
 * the depth / segmentation renders of physics.render(camera_id=..., depth=True | segmentation=True) on the reference's cameras
 * (so100_task.py:107-112, scene_pbr.xml:70-71,113,138-139); RGB, textures and visual-only meshes are not rendered.
 *
 * so101_set_hull_planes: the facet planes of the mesh geoms' convex hulls, geom frame: planes[n][4] = unit outward normal n and offset d with
 * n . x + d <= 0 inside; plane_adr[ngeom + 1] = each geom's range (HOST arrays, copied; so101_sim_amd.model.meshes.hull_planes computes them).
 * Checked before the upload - SO101_ERR_ARG with a message naming the geom: non-mesh geoms have empty ranges, a mesh geom has at least 4 planes,
 * | |n| - 1 | <= 1e-4, every vertex of the hull has n . v + d <= 1e-5, every plane has a vertex within 1e-5 of it. */
int so101_set_hull_planes(so101_sim* sim, const float* planes, const int32_t* plane_adr);
typedef struct {
  int32_t body;       /* so101_render: -1 world, 0..5 arm link, 6..7 free prop (the numbering of the model's geom_dyn); so101_tree_render: -1 or 0
                         world, 1 .. nbody - 1 a body of the tree (the blob's body numbering) */
  float pos[3];       /* camera frame in that body's frame */
  float mat[9];       /* row-major, columns x (right), y (up), z; the camera looks along -z (MuJoCo's convention) */
  float fovy_deg;     /* vertical field of view, 0 < fovy_deg < 180 */
} so101_camera;
/* Renders ncam cameras (HOST array, 1..8) at height x width (1..4096 each) for n_render envs from the qpos in the bound buffers; asynchronous on
 * `hip_stream`, changes no state.  env_index: DEVICE array of n_render env indices, or NULL for envs 0 .. n_render - 1 (n_render = n_envs: all).
 * depth / seg: DEVICE arrays [n_render][ncam][height][width], either may be NULL.  Pixel (r, c): the ray from the camera position along the
 * camera-frame direction ((c + 0.5 - W/2) s, -(r + 0.5 - H/2) s, -1), s = 2 tan(fovy / 2) / H; depth = the ray parameter of the nearest hit (the
 * distance along the optical axis), +inf without one; seg = the geom index, -1 without one; equal depths: the lower index.  A plane is hit from its
 * front only and clipped to its positive sizes, a geom that contains the camera position is invisible.  A pixel's bits depend on the env's qpos,
 * the camera and (r, c, height, width) only.  SO101_ERR_STATE while the scene has mesh geoms and so101_set_hull_planes has not been called. */
int so101_render(so101_sim* sim, const so101_camera* cams, int ncam, int height, int width, const int32_t* env_index, int n_render,
                 float* depth, int32_t* seg, void* hip_stream);

/* ---- colour cameras (csrc/so101_shade.hpp): so101_render with two more outputs per pixel - the world-frame unit normal of the surface the ray
 * hit and a Lambert-shaded flat colour.  What is drawn is the COLLISION geometry of so101_render, one colour per geom, lit by directional lights:
 * this is not MuJoCo's renderer - no textures, shadows, specular term, visual-only meshes or positional lights.  Stands in for the RGB image of
 * physics.render(camera_id=...) that the reference's observation.images.<camera> carry (scripts/so101_lerobot_wrapper.py:85-98).
 *
 * Pixel: ray, hit, depth and seg are so101_render's, bit for bit.  normal: the outward normal of the feature through which the ray enters the hit
 * geom, geom frame, rotated by the geom's world matrix, unit - plane +z; sphere x / |x| at the hit point x; capsule x minus its projection onto the
 * axis segment, normalised; cylinder the side (radial) if the side's entry parameter is >= the slab's, else the cap (0, 0, -sign(d.z)); box the axis
 * whose slab entry parameter is largest (x before y before z at equal values), -sign(d[axis]) along it; mesh the hull plane with the largest
 * t = -num / den among planes with den < 0 (the first in plane order at equal t); no hit: 0.  rgb: v_k = clamp(C_g[k] (ambient[k] +
 * sum_l diffuse_l[k] max(0, -n . u_l)), 0, 1), byte (uint8)(255 v_k + 0.5), C_g the colour of the hit geom, u_l the unit world direction light l
 * travels (`dir`; for a light flagged `headlight` the camera's viewing direction, `dir` unread); no hit: `background`, converted the same way.
 * A pixel's bits depend on the env's qpos, the camera, (r, c, height, width), that env's colours and the shading only.
 *
 * geom_rgb: DEVICE [ngeom][3], or [n_envs][ngeom][3] with rgb_per_env != 0 (entry i uses the row of env env_index[i]); caller-owned, values are
 * clamped by the formula, not checked.  out: HOST struct of DEVICE pointers.  Asynchronous on `hip_stream`, changes no state.  Errors: those of
 * so101_render for the shared arguments, and SO101_ERR_ARG (with a message) for NULL shading, geom_rgb or out; no output pointer at all; nlight
 * outside 0 .. SO101_MAX_LIGHTS; a non-headlight dir whose length is not within 1e-4 of 1; a non-finite or negative ambient, diffuse or
 * background. */
#define SO101_MAX_LIGHTS 4
typedef struct {
  float ambient[3], background[3];
  int32_t nlight;                                   /* 0 .. SO101_MAX_LIGHTS */
  struct { float dir[3]; float diffuse[3]; int32_t headlight; } light[SO101_MAX_LIGHTS];
} so101_shading;                                    /* HOST, copied */
typedef struct {
  uint8_t* rgb;      /* [n_render][ncam][height][width][3] */
  float*   normal;   /* [n_render][ncam][height][width][3] */
  float*   depth;    /* as so101_render */
  int32_t* seg;      /* as so101_render */
} so101_color_out;                                  /* DEVICE pointers, any may be NULL, not all */
int so101_render_color(so101_sim* sim, const so101_camera* cams, int ncam, int height, int width, const int32_t* env_index, int n_render,
                       const so101_shading* shading, const float* geom_rgb, int rgb_per_env, const so101_color_out* out, void* hip_stream);

/* ---- Cartesian tool control (csrc/so101_tool_chain.hpp): the pose and Jacobian of a frame fixed to an arm link, and the inverse map, for thousands of
 * envs per call on the device.  so101_tool_pose stands in for physics.named.data.site_xpos / site_xmat and mujoco.mj_jacSite of the reference;
 * so101_tool_ik for dm_control's qpos_from_site_pose (dm_control/utils/inverse_kinematics.py), which the reference's data generator approximates by
 * hand (examples/automated_lerobot_dataset_generator.py:180 _inverse_kinematics_approximate).  These are the calls of the SO100 engine; the general-tree engine (ALOHA, Dining) has so101_tree_tool_pose /
 * so101_tree_tool_ik below.  Additions: the ABI number stays. */
typedef struct {
  int32_t body;       /* 0..5: arm link in chain order, the numbering of so101_camera.body */
  float pos[3];       /* the tool frame in that body's frame */
  float mat[9];       /* row-major, orthonormal (|M^T M - I| <= 1e-4 entrywise) */
} so101_tool;
typedef struct {
  int32_t mode;       /* what the solve drives to zero besides the position error: 0 nothing, 1 the angle between the tool's z axis and the target's,
                         2 the full orientation error */
  int32_t max_iters;  /* 0..1000 */
  float tol_pos;      /* metres, > 0 */
  float tol_rot;      /* radians, > 0 */
  float rot_weight;   /* metres per radian: weight of the orientation rows, > 0 */
  float damping;      /* >= 0, added to the error-proportional damping */
  float max_step;     /* radians: largest joint change of one iteration, > 0 */
  float q_lo[6], q_hi[6];   /* joint limits the iterates are clamped to, q_lo <= q_hi */
} so101_ik_config;
/* mode 1, 60 iterations, 1e-4 m, 1e-3 rad, weight 0.1, damping 1e-6, 0.5 rad per iteration, the model's jnt_range */
int so101_ik_default_config(const so101_sim* sim, so101_ik_config* cfg);
/* Tool pose of n entries: pos[n][3] = xpos_b + R_b tool.pos, mat[n][9] = R_b tool.mat (row-major) and jac[n][6][6] (row-major, MuJoCo's mj_jacSite:
 * rows 0-2 jacp, rows 3-5 jacr; column j = (a_j x (p - o_j), a_j) with a_j the world axis of joint j and o_j the world origin of arm link j; columns of
 * joints beyond the tool's link are zero).  Any output may be NULL, but not all.  q: DEVICE [n][6] joint angles, row-major like `action`, or NULL = the
 * arm joints of the bound qpos; env_index (only with q == NULL): DEVICE array of n env indices, NULL = envs 0 .. n - 1 (then n <= n_envs).  An
 * env_index entry outside the batch reads nothing and gives NaN outputs.  Asynchronous on `hip_stream`, changes no state.  SO101_ERR_ARG (with a
 * message): NULL handle or tool, body outside 0..5, non-orthonormal mat, n outside 1 .. 2^26 (or > n_envs when reading the bound state), env_index together
 * with q, no output.  SO101_ERR_STATE: q == NULL and no state bound. */
int so101_tool_pose(so101_sim* sim, const so101_tool* tool, const float* q, const int32_t* env_index, int n, float* pos, float* mat, float* jac,
                    void* hip_stream);
/* Damped least-squares inverse kinematics, one independent solve per entry: target_pos[n][3], target_mat[n][9] (row-major; may be NULL in mode 0),
 * q_init[n][6] or NULL = the bound qpos (then env_index as above), q_out[n][6], residual[n][2] = |e_p|, |e_r| at q_out (may be NULL), info[n] = the
 * iterations used if converged, -1 if not (may be NULL).  The algorithm:
 *   q = clamp(q_init, q_lo, q_hi)
 *   for it = 0 .. max_iters:
 *     p, M, J = tool pose and Jacobian at q;  e_p = p_target - p
 *     e_r = 0 (mode 0) | rotation vector of the smallest rotation taking M[:,2] to M_target[:,2] (mode 1) | rotation vector of M_target M^T,
 *           angle in [0, pi] (mode 2)
 *     if |e_p| <= tol_pos and |e_r| <= tol_rot: info = it, stop;   if it == max_iters: info = -1, stop
 *     Jr' = 0 (mode 0) | (I - z z^T) Jr, z = M[:,2] (mode 1: the spin about z is left free) | Jr (mode 2)
 *     Jw = [Jp ; w Jr'], e = [e_p ; w e_r], w = rot_weight
 *     dq = Jw^T (Jw Jw^T + (e . e + damping) I)^-1 e          (6 x 6 Cholesky without pivoting, in registers)
 *     if max |dq_j| > max_step: dq *= max_step / max |dq_j|
 *     q = clamp(q + dq, q_lo, q_hi)
 * A joint beyond the tool's link has a zero column and keeps clamp(q_init) (for a tool on Fixed_Jaw: the jaw).  A non-finite target gives info = -1 and
 * q_out = clamp(q_init); an env_index entry outside the batch info = -1 and NaN q_out and residual.  At an angle of exactly pi the rotation axis is
 * undefined; csrc/so101_tool_common.hpp says which one is taken.  An entry's output bits depend on its own inputs, the tool and the configuration only - not on the
 * other entries of the call or on n.  Asynchronous on `hip_stream`, changes no state.  SO101_ERR_ARG as for so101_tool_pose and for: NULL config,
 * target_pos or q_out, mode outside 0..2, max_iters outside 0..1000, tol_pos / tol_rot / rot_weight / max_step <= 0, damping < 0, q_lo > q_hi, a
 * missing target_mat in modes 1 and 2.  SO101_ERR_STATE: q_init == NULL and no state bound. */
int so101_tool_ik(so101_sim* sim, const so101_tool* tool, const so101_ik_config* cfg, const float* target_pos, const float* target_mat,
                  const float* q_init, const int32_t* env_index, int n, float* q_out, float* residual, int32_t* info, void* hip_stream);

/* ---- contact sensing (csrc/so101_contacts.hpp): the contact list of an env's CURRENT bound state (qpos, qvel, ctrl, warmstart) and its reduction
 * over pairs of geom groups, for thousands of envs per call on the device.  Stands in for physics.data.contact / physics.data.ncon and the
 * reference tasks' _touching(geoms_a, geoms_b) loops over it (so100_hand_over.py:291-313), and with forces != 0 for mujoco.mj_contactForce.  The
 * pass is mj_forward at the bound state cut down to the report: kinematics and collision for the geometry; with forces != 0 also the mass
 * matrix, the smooth dynamics, the constraint rows and the configured solver (the iterations, tolerance and warmstart of so101_debug_forward) -
 * with forces == 0 none of that runs.  So the forces are those of a forward pass at the current state, NOT the impulses of the last substep.
 * SO100 engine; so101_tree_contacts below is the general-tree engine's.  Additions: the ABI number stays.
 *
 * A group is a 128-bit mask over geoms; a contact belongs to pair (a, b) if one of its geoms is in a and the other in b.  The order
 * "geom1 in a, geom2 in b" is tried first, "geom2 in a, geom1 in b" second: a contact for which both hold (overlapping groups) counts once,
 * with the sign of the first.  pair_force: with R the contact's frame (rows) and f its force, the constraint force acts on geom2's body along
 * the normal from geom1 to geom2, so the contact adds +R^T f[0:3] when group A holds geom2 and -R^T f[0:3] when it holds geom1: the net
 * world-frame force ON group A.  Swapping a and b negates pair_force (bit for bit when no contact holds both orders) and changes nothing else.
 *
 * The list is the step's: at most so101_max_contacts() contacts per env, in the step's order; an env with more keeps one contact per touching
 * geom pair (the capacity rule of event 7).  flags = diag word 4 of THIS pass: 1 candidate overflow, 2 contact overflow, 128 reduced to one
 * contact per pair (with forces != 0 also what the solve raises).  frame is the full MuJoCo contact.frame; force is the contact's force in that
 * frame, the entries beyond its dim zero (csrc/so101_contacts.hpp says where both are read).  Slots at or beyond count: geoms -1, dist +inf,
 * the other floats 0.  An env_index entry outside the batch reads nothing: count -1, flags 0, geoms -1, pair_count 0, every float output NaN
 * (the convention of so101_tool_pose).  An entry's output bits depend on its env's state, forces, the solver settings and (the pair outputs)
 * its pair only - not on n or the other entries.  Asynchronous on `hip_stream`, changes no state - the warmstart included.
 *
 * env_index: DEVICE array of n env indices, or NULL for envs 0 .. n - 1.  pairs: HOST array of npair pairs, copied.  out: HOST struct of
 * DEVICE pointers.  SO101_ERR_ARG (with a message in so101_last_error): NULL handle or out; no output pointer at all; n outside 1 .. 2^26, or
 * n > n_envs with env_index == NULL; npair outside 0 .. SO101_TOUCH_MAX_PAIRS; npair > 0 with NULL pairs; a pair output with npair == 0; an
 * empty group; a group bit at or beyond ngeom; force, pair_normal or pair_force with forces == 0.  SO101_ERR_STATE: no state bound, or a
 * model with more than 128 geoms. */
#define SO101_TOUCH_MAX_PAIRS 16
typedef struct { uint32_t a[4], b[4]; } so101_geom_pair;   /* bit (g & 31) of word g >> 5: geom g belongs to the group; ngeom <= 128 */
typedef struct {
  int32_t* count;        /* [n]        contacts of the env, -1 for an env_index outside the batch */
  int32_t* flags;        /* [n]        the overflow bits of diag word 4 for THIS pass (candidate overflow, contact overflow, reduced to one per pair) */
  int32_t* geom;         /* [n][C][2]  geom1, geom2;  C = so101_max_contacts() */
  float*   dist;         /* [n][C] */
  float*   pos;          /* [n][C][3] */
  float*   frame;        /* [n][C][9]  rows: normal (geom1 -> geom2), tangent 1, tangent 2: MuJoCo's contact.frame */
  float*   force;        /* [n][C][6]  mj_contactForce: the contact's force in its frame, entries beyond its dim zero; needs forces != 0 */
  int32_t* pair_count;   /* [n][npair] */
  float*   pair_dist;    /* [n][npair] minimum dist, +inf without a contact */
  float*   pair_normal;  /* [n][npair] sum of f[0]; needs forces */
  float*   pair_force;   /* [n][npair][3] world frame, the force ON group A; needs forces */
} so101_contact_out;       /* DEVICE pointers, any may be NULL, not all */
int so101_contacts(so101_sim* sim, const int32_t* env_index, int n, int forces,
                   const so101_geom_pair* pairs /* HOST, npair of them */, int npair,
                   const so101_contact_out* out, void* hip_stream);

/* ---- proximity sensing (csrc/so101_proximity.hpp): how far apart two groups of geoms are while they do not touch - MuJoCo's mj_geomDistance /
 * <distance> sensor, batched.  Per entry i and pair p: over every geom pair of the model's admitted pair list (the list the broadphase walks:
 * no same-body and no excluded pairs) with one geom in group a and the other in b, the smallest signed distance.  Separated geoms: the
 * Euclidean gap of the surfaces (GJK, spheres and capsules as core plus radius), >= 0.  Penetrating geoms: the smallest contact dist of the
 * step's narrowphase for that geom pair (< 0, the number so101_contacts' pair_dist gives), flags bit 1.  geom: the winning geom pair, the
 * a-side geom first.  point: the closest point on the a-side geom and on the b-side geom, world frame; for a penetrating pair the contact
 * position offset by -+ dist / 2 along the normal.  normal: unit vector from the a point to the b point; for a penetrating pair the contact
 * normal oriented from a to b.  Nothing below max_dist (or no admitted pair): dist = max_dist, geom -1, point and normal 0, flags bit 4 (what
 * mj_geomDistance does with distmax).  flags: 1 penetrating, 2 the distance iteration hit its cap on the winning pair (the value is an upper
 * bound), 4 nothing within max_dist, 8 (with 4) the entry's env index is outside the batch.  Ties go to the pair that comes first in the
 * pair list.  queries: exact pair queries run for the entry and pair (the rest was culled by bounding spheres).
 *
 * q: DEVICE [n][6] arm joint angles (qpos[0:6], the convention of so101_tool_pose) or NULL: entry i is evaluated with the props of env
 * env_index[i] where they are and the arm at q[i]; nothing bound is read for the arm's angles then and nothing bound is ever written - qpos, qvel,
 * ctrl and the warmstart stay as they are.  env_index may repeat an env: K waypoints against one env in one call.  An entry's output bits
 * depend on its env's state, q[i], its pair and max_dist only.  Asynchronous on `hip_stream`.  This is the SO100 engine's; so101_tree_proximity below is the general-tree engine's.  An addition: the ABI number stays.
 *
 * env_index: DEVICE array of n env indices, or NULL for envs 0 .. n - 1.  pairs: HOST array of npair pairs, copied.  out: HOST struct of
 * DEVICE pointers.  SO101_ERR_ARG (with a message in so101_last_error): NULL handle or out; no output pointer at all; n outside 1 .. 2^26, or
 * n > n_envs with env_index == NULL; npair outside 1 .. SO101_TOUCH_MAX_PAIRS; NULL pairs; an empty group; a group bit at or beyond ngeom;
 * max_dist not a finite number in (0, 10].  SO101_ERR_STATE: no state bound. */
typedef struct {
  float*   dist;     /* [n][npair] */
  int32_t* geom;     /* [n][npair][2]    a-side geom, b-side geom; -1 with flags bit 4 */
  float*   point;    /* [n][npair][2][3] */
  float*   normal;   /* [n][npair][3] */
  int32_t* flags;    /* [n][npair] */
  int32_t* queries;  /* [n][npair] */
} so101_proximity_out;     /* DEVICE pointers, any may be NULL, not all */
int so101_proximity(so101_sim* sim, const int32_t* env_index, int n, const float* q /* DEVICE [n][6] or NULL */,
                    const so101_geom_pair* pairs /* HOST, npair of them */, int npair, float max_dist,
                    const so101_proximity_out* out, void* hip_stream);

const char* so101_last_error(const so101_sim* sim);

/* ---- general-tree engine (csrc/so101_tree.hpp): models outside the SO100 topology - the ALOHA hand-over scenes of
 * so101_sim/tasks/hand_over.py (two 8-dof arms with slide fingers coupled by joint equalities, position actuators, joint
 * damping; reference model so101_sim/assets/aloha/aloha_pbr.xml).  The blob is the f32 blob of
 * so101_sim_amd.model.scenes.compile_aloha_scene / compile_dining_scene; limits: 32 bodies, 16 actuators and, per build, 32 dofs /
 * 128 geoms / 64 contacts / 384 rows (ALOHA hand-over) or 64 dofs / 256 geoms / 160 contacts / 960 rows (Dining).
 * Physics entry points only so far (what dm_control's physics.step() does for these scenes); same conventions as above:
 * device pointers, env-fastest struct-of-arrays state [dim][n_envs], asynchronous on `hip_stream`. */
typedef struct so101_tree so101_tree;
int so101_tree_create(const void* model_blob, size_t blob_bytes, int n_envs, int hip_device, so101_tree** out);
void so101_tree_destroy(so101_tree* sim);
/* dims[16] = nq, nv, nu, nbody, ngeom, floats per env of so101_tree_debug_forward, contact capacity; then the layout of that row for the
 * handle's build - offsets of bias, qacc_smooth, qacc, body positions, mass matrix, contacts, normal forces, the row stride of the mass
 * matrix - and the build itself (32 or 64: so101_tree_create takes the 32-dof / 128-geom / 64-contact build whenever the model fits it,
 * otherwise the 64-dof / 256-geom / 160-contact one of the Dining scenes) */
int so101_tree_dims(const so101_tree* sim, int* dims);
/* What the last so101_tree_step of this handle enqueued, as the library counted it (not a host-side copy of the rule): out[4] = env slices,
 * kernel launches, memsets, path (0: no step yet, 1: the single kernel k_tree_step, 2: the launch chain).  A step that returns SO101_ERR_HIP
 * leaves the counts of the last step that was enqueued whole.  bench.py reports it as evidence. */
int so101_tree_last_plan(const so101_tree* sim, int* out);
int so101_tree_bind_state(so101_tree* sim, float* qpos, float* qvel, float* ctrl, float* warmstart);
/* solver_iterations <= 0 / solver_tolerance < 0 keep the model's (100, 1e-8) */
int so101_tree_configure(so101_tree* sim, int solver_iterations, float solver_tolerance);
/* n_substeps of mj_step (forward dynamics with contacts and the Newton solver, Euler with implicit joint damping) on the
 * bound state, ctrl as bound */
int so101_tree_physics(so101_tree* sim, int n_substeps, void* hip_stream);
/* forward dynamics at the bound state without integrating; out[n_envs][dims[5]] floats: counts (contacts, rows, solver
 * iterations, candidates, flags, scalar rows) at 0, then bias, qacc_smooth, qacc, body positions, the mass matrix, contacts [.][10]
 * (position, normal, distance, geom1, geom2, condim) and normal forces at the offsets so101_tree_dims reports (32-dof build: 8, 40, 72,
 * 104, 200 [32][32], 1224, 1864) */
int so101_tree_debug_forward(so101_tree* sim, float* out, void* hip_stream);
/* out[n_envs][8] int32 of the last so101_tree_physics / so101_tree_step / so101_tree_reset: contacts, rows, solver iterations,
 * candidates, flags (1 candidate overflow, 2 contact overflow, 4 row overflow: contacts dropped, 8 physics diverged, 16 container
 * placement rejected 20 times, 32 settle budget used up); after so101_tree_step word 5 holds the state of the contact-sequence reward */
int so101_tree_get_diag(so101_tree* sim, int32_t* out, void* hip_stream);
/* ---- env layer of the hand-over scenes on this engine (HandOverBanana / HandOverPen of the reference's task_suite.py:60-61):
 * before_step with the gripper unit conversion (aloha2_task.py:316-349), n_substeps of physics, the observables of
 * aloha2_task.py:386-444 with their 0.1 s delay, the overlap reward and termination of hand_over.py:246-284 / aloha2_task.py:355-367,
 * reset = home pose + prop placement + settle (aloha2_task.py:369-383, hand_over.py:208-236).  Caller-owned per-env arrays
 * (device, env-fastest): ring_pos [joints_delay_steps][npos][n_envs], ring_vel [joints_delay_steps][nvel][n_envs] (npos = nu = 14,
 * nvel = 16 for ALOHA; the delay as configured, 5 by default; with a delay of 0 the pointers are still required but never touched),
 * ep_return, step_count, episode.  Observation row of so101_tree_step, so101_tree_obs_dim() = 3 npos + 2 nvel floats per env:
 *   joints_pos (delayed) | joints_vel (delayed) | undelayed_joints_pos | undelayed_joints_vel | commanded_joints_pos
 * step_type 0 FIRST (the call after a LAST resets the env and ignores the action), 1 MID, 2 LAST; a physics error ends the
 * episode with reward 0 and discount 0.  Reset happens inside the step call: a copy when the settled-state store or the reset prefetch
 * (prefetch_resets) holds the episode, placement + settle in place otherwise. */
typedef struct {
  int n_substeps;            /* physics steps per control step (10) */
  int last_step;             /* control step on which the time limit ends the episode */
  int settle_max_substeps;   /* settle budget of a reset (1000) */
  int terminate_on_success;
  int solver_iterations;     /* <= 0: the model's */
  float solver_tolerance;    /* < 0: the model's */
  uint64_t seed, env_id_base;
  int reward_mode;           /* 0 overlap boxes (HandOver's default; Dining 'bbox'), 1 contact sequence (reward_based_on_overlap = False,
                                hand_over.py:286-338), 2 object touches receptacle (Dining 'contact', dining_place_in_container.py:126-154) */
  int reward_requires_handover;   /* mode 1: start the sequence at "right gripper touches the object" instead of at its last state */
  int joints_delay_steps;    /* delay of joints_pos / joints_vel in CONTROL steps (joints_observation_delay_secs / control_timestep,
                                aloha2_task.py:153-155,236-243); < 0: the reference's default 5 (0.1 s); 0: undelayed; at most 64 */
  int physics_delay_steps;   /* delay of delayed_physics_state (image_observation_delay_secs, aloha2_task.py:157-159,244-251); < 0: 15 (0.3 s) */
  int prefetch_resets;       /* != 0: the settled initial state of every env's NEXT episode is computed on an internal low-priority stream beside
                                the stepping kernels (library-owned cache + a second per-env scratch); a reset that finds its entry copies it, one
                                that does not settles in place - the same bits either way.  so101_tree_configure_env / so101_tree_destroy join it */
  int pipeline;              /* != 0: so101_tree_step runs as a launch chain - per substep one launch with a wavefront per candidate pair of the whole
                                batch (the narrowphase) and one with a wavefront per env (everything else) - instead of one kernel; the same bits
                                either way (the contact rewards add one narrowphase launch on the post-step state).  At most 63 substeps; above, the single kernel */
} so101_tree_config;
int so101_tree_obs_dim(const so101_tree* sim);
int so101_tree_bind_env(so101_tree* sim, float* ring_pos, float* ring_vel, float* ep_return, int32_t* step_count, int32_t* episode);
int so101_tree_configure_env(so101_tree* sim, const so101_tree_config* cfg);
/* physics_state / delayed_physics_state (aloha2_task.py:244-251,441-444: qpos | qvel, and its copy of physics_delay_steps control
 * steps ago, padded with the reset state) written by so101_tree_step / so101_tree_reset / so101_tree_begin_episode: caller-owned
 * device buffers ring [physics_delay_steps][nq + nv][n_envs] (env-fastest), physics_state [n_envs][nq + nv], delayed [n_envs][nq + nv];
 * all NULL switches the outputs off.  Replaces the host-side line of rounds 3 (reference test: aloha2_task_test.py:136-173). */
int so101_tree_bind_physics_state(so101_tree* sim, float* ring, float* physics_state, float* delayed);
int so101_tree_reset(so101_tree* sim, const uint8_t* mask, void* hip_stream);
/* Settled-state store, as so101_compute_settled / so101_set_settled_store above: placement + settle of episodes first_episode ..
 * first_episode + count - 1 of every env into caller-owned device tables qpos [count][nq][n_envs], qvel / warmstart [count][nv][n_envs],
 * flags [count][n_envs] (one launch per episode at the width of the machine), and their use by the resets of those episodes - copies,
 * bit-identical to settling in place.  The tables depend on seed, env_id_base, n_envs and the solver settings; count = 0 detaches. */
int so101_tree_compute_settled(so101_tree* sim, int first_episode, int count, float* qpos, float* qvel, float* warmstart, int32_t* flags, void* hip_stream);
int so101_tree_set_settled_store(so101_tree* sim, int first_episode, int count, const float* qpos, const float* qvel, const float* warmstart, const int32_t* flags);
/* PropPlacer(settle_physics=True) alone, for callers that draw the placements themselves: physics steps on the bound state with the
 * one-dof joints held until the props rest (|qvel| < 1e-3, |qacc| < 1e-2) or settle_max_substeps is used up (diag flag 32) */
int so101_tree_settle(so101_tree* sim, void* hip_stream);
/* adopt the bound state (qpos, qvel, ctrl) as the post-reset state of a new episode: delay lines filled with it, counters cleared */
int so101_tree_begin_episode(so101_tree* sim, void* hip_stream);
int so101_tree_step(so101_tree* sim, const float* action /*[n_envs][nu]*/, float* obs, float* reward, float* discount, uint8_t* step_type,
                    void* hip_stream);
/* ---- depth and segmentation cameras of this engine: so101_set_hull_planes / so101_render above, word for word, on a tree handle - the same
 * image kernel fed by this engine's kinematics.  Stands in for the depth / segmentation renders of the cameras the reference turns on for these
 * tasks (aloha2_task.py:151-232 cameras=('overhead_cam',), scene_pbr.xml:74-77, aloha_pbr.xml:122-123,172,256); RGB is not rendered.
 *
 * so101_tree_set_hull_planes: same arrays, same checks, same error messages (naming the geom) as so101_set_hull_planes.
 * so101_tree_render: a camera's `body` is a tree body id (-1 or 0: fixed to the world).  source selects the qpos the kinematics runs on:
 * 0 = the bound state (so101_tree_bind_state), 1 = the `delayed` buffer of so101_tree_bind_physics_state (its first nq entries per env: what the
 * reference's delayed camera observables look at).  Pixel definition, argument limits, tie rule and "a pixel's bits depend on that env's qpos,
 * the camera and (r, c, height, width) only" are those of so101_render; asynchronous on `hip_stream`, changes no state.  SO101_ERR_STATE while
 * the scene has mesh geoms and so101_tree_set_hull_planes has not been called, and for source 1 without a bound physics-state line;
 * SO101_ERR_ARG for a body outside -1 .. nbody - 1, a bad fovy_deg or another source. */
int so101_tree_set_hull_planes(so101_tree* sim, const float* planes, const int32_t* plane_adr);
int so101_tree_render(so101_tree* sim, const so101_camera* cams, int ncam, int height, int width, const int32_t* env_index, int n_render,
                      int source, float* depth, int32_t* seg, void* hip_stream);
/* ---- colour cameras of this engine: so101_render_color above, word for word, on a tree handle (`source` as in so101_tree_render; geom_rgb rows
 * have the handle's ngeom, dims[4]); the error messages carry the name so101_tree_render_color. */
int so101_tree_render_color(so101_tree* sim, const so101_camera* cams, int ncam, int height, int width, const int32_t* env_index, int n_render,
                            int source, const so101_shading* shading, const float* geom_rgb, int rgb_per_env, const so101_color_out* out,
                            void* hip_stream);
/* ---- Cartesian tool control of this engine (csrc/so101_tool_chain.hpp): so101_tool_pose / so101_tool_ik above for a frame on any articulated body of
 * a general-tree model - the grippers and fingers of the two ALOHA arms (the sites left/gripper, right/gripper and the four finger sites of
 * aloha_pbr.xml), on both builds of the engine.  The chain of a tool is the bodies between the world and the tool's body that carry a hinge or slide
 * joint, root first: ncol <= 8 columns.  Bodies without a joint (the arms' base_link and gripper_base) are folded into fixed transforms on the host.
 * Additions: the ABI number stays. */
typedef struct {
  int32_t body;       /* 1 .. nbody - 1: body id, blob numbering (meta "body_names") */
  float pos[3];       /* the tool frame in that body's frame */
  float mat[9];       /* row-major, orthonormal (|M^T M - I| <= 1e-4 entrywise) */
} so101_tree_tool;
typedef struct {
  int32_t mode, max_iters;        /* as so101_ik_config */
  float tol_pos, tol_rot, rot_weight, damping, max_step;
  uint32_t free_mask;             /* bit k set: column k of the chain is solved for; clear: its column of Jw is zero and the joint keeps clamp(q_init) */
  float q_lo[8], q_hi[8];         /* per column; entries at and beyond ncol are ignored */
} so101_tree_ik_config;
/* The columns of a tool on `body`: dof[k] (index into qvel), qposadr[k] (index into qpos) and jnt_type[k] (1 hinge, 3 slide), root first; each
 * array has room for 8 entries and may be NULL.  Returns ncol (1 .. 8), or SO101_ERR_ARG with a message for a body outside 1 .. nbody - 1, a body with
 * no joint above it (the table), a body whose chain contains a free joint (the props) and a chain longer than 8. */
int so101_tree_tool_chain(const so101_tree* sim, int body, int32_t* dof, int32_t* qposadr, int32_t* jnt_type);
/* mode 1, 60 iterations, 1e-4 m, 1e-3 rad, weight 0.1, damping 1e-6, 0.5 per iteration, the model's jnt_range of the chain's joints, free_mask = the
 * hinge columns (slide joints - the fingers - are held).  Errors as so101_tree_tool_chain. */
int so101_tree_ik_default_config(const so101_tree* sim, int body, so101_tree_ik_config* cfg);
/* so101_tool_pose for this engine: pos[n][3], mat[n][9] and jac[n][6][ncol] (row-major; column k belongs to dof[k] of so101_tree_tool_chain: hinge
 * (a x (p - o), a), slide (a, 0), with a the world axis of the joint and o the world origin of its body).  q: DEVICE [n][ncol] joint values of the
 * chain, root first, or NULL = the bound qpos ([nq][n_envs]) at the chain's qposadr, of env env_index[i] (NULL: env i, then n <= n_envs).  An env_index
 * entry outside the batch reads nothing and gives NaN outputs.  Asynchronous on `hip_stream`, changes no state.  SO101_ERR_ARG (with a message) as
 * for so101_tool_pose and so101_tree_tool_chain; SO101_ERR_STATE: q == NULL and no state bound. */
int so101_tree_tool_pose(so101_tree* sim, const so101_tree_tool* tool, const float* q, const int32_t* env_index, int n, float* pos, float* mat, float* jac,
                         void* hip_stream);
/* so101_tool_ik for this engine - the algorithm written down there, word for word, over ncol columns instead of 6 and with the free_mask: q_init[n][ncol]
 * or NULL = the bound qpos, q_out[n][ncol], residual[n][2], info[n].  A non-finite target gives info = -1 and q_out = clamp(q_init); an env_index entry
 * outside the batch info = -1 and NaN q_out and residual.  An entry's output bits depend on its own inputs, the tool and the configuration only - not
 * on the other entries of the call or on n.  Asynchronous on `hip_stream`, changes no state.  SO101_ERR_ARG as for so101_tree_tool_pose, the checks of
 * so101_tool_ik on the configuration (q_lo <= q_hi over the chain's columns), and free_mask bits at or above ncol. */
int so101_tree_tool_ik(so101_tree* sim, const so101_tree_tool* tool, const so101_tree_ik_config* cfg, const float* target_pos, const float* target_mat,
                       const float* q_init, const int32_t* env_index, int n, float* q_out, float* residual, int32_t* info, void* hip_stream);
/* ---- contact sensing of this engine (k_tree_contacts of csrc/so101_tree_kernels.hpp): so101_contacts above on a tree handle, for both builds - the same semantics
 * and conventions with this engine's stages and capacity.  The pass is so101_tree_debug_forward's cut down to the report: kinematics and collision for
 * the geometry; with forces != 0 also the mass matrix, the bias forces, the smooth dynamics, the constraint rows and the Newton solve with the handle's
 * iterations and tolerance (so101_tree_configure) - with forces == 0 none of that runs.  Its numbers are so101_tree_debug_forward's bit for bit.
 * Stands in for looping over physics.data.contact in the contact-sequence reward (hand_over.py:286-338) and the Dining `contact` reward
 * (dining_place_in_container.py:126-154), and with forces for mujoco.mj_contactForce.
 *
 * so101_contact_out is reused unchanged with C = the handle's contact capacity, dims[6] of so101_tree_dims (64 or 160).  A group is a 256-bit mask
 * over geoms, in both builds.  Pair membership, the order rule ("geom1 in a, geom2 in b" first; a contact holding both orders counts once, with the
 * sign of the first), the sign of pair_force (the net world-frame force ON group A), the fill values of slots at or beyond count (geoms -1, dist
 * +inf, the other floats 0) and the convention for an env_index entry outside the batch (count -1, flags 0, geoms -1, pair_count 0, every float NaN)
 * are those of so101_contacts.
 *
 * The capacity rule is THIS engine's: the list is the step's, in the step's order, and it ENDS at the first candidate pair whose contacts do not fit
 * the capacity (flag 2) - there is no reduction to one contact per pair.  flags = the engine's flag word of THIS pass, started at 0: 1 candidate
 * overflow, 2 contact overflow, and with forces != 0 also 4: the constraint rows of the last contacts did not fit the row capacity and those contacts
 * were left out of the solve.  count and the per-contact geometry are always those of the collision stage, so the geometry is the same bit for bit
 * with and without forces; a contact that got no rows reports zero force and adds nothing to pair_normal / pair_force.
 *
 * An entry's output bits depend on its env's state, forces, the solver settings and (the pair outputs) its pair only - not on n or the other entries;
 * env_index may name an env more than once.  Asynchronous on `hip_stream` (with forces != 0 as ceil(n / n_envs) launches), changes no state - the
 * warmstart included.  env_index: DEVICE, or NULL for envs 0 .. n - 1; pairs: HOST, copied; out: HOST struct of DEVICE pointers.  SO101_ERR_ARG with
 * the messages of so101_contacts under the name so101_tree_contacts (ngeom is the handle's, dims[4]); SO101_ERR_STATE: no state bound. */
typedef struct { uint32_t a[8], b[8]; } so101_tree_geom_pair;   /* 256-bit groups, bit (g & 31) of word g >> 5; both builds take this struct */
int so101_tree_contacts(so101_tree* sim, const int32_t* env_index, int n, int forces,
                        const so101_tree_geom_pair* pairs /* HOST, npair of them */, int npair,
                        const so101_contact_out* out, void* hip_stream);

/* ---- proximity sensing of this engine (k_tree_proximity of csrc/so101_tree_kernels.hpp): so101_proximity above on a tree handle, for both builds - the
 * same semantics, conventions and flag meanings, the same distance code (csrc/so101_proximity_core.hpp), so101_proximity_out reused unchanged.  A group
 * is a 256-bit mask over geoms (so101_tree_geom_pair).  The pass is load the env's state, the columns of q, kinematics; no dynamics runs.  A
 * penetrating geom pair goes to this engine's narrowphase on geoms loaded as its collision stage loads them: its dist is so101_tree_contacts'
 * pair_dist for that pair at that state, bit for bit, and flags bit 1 is set where that call reports a contact.
 *
 * q and q_adr: the arms are one-dof joints anywhere in qpos and a caller holds q in the column order of a tool's chain (what so101_tree_tool_ik
 * returns), so q is DEVICE [n][ncol] with q_adr HOST [ncol], the qpos address of each column (so101_tree_tool_chain's qposadr, or any hinge /
 * slide joint's), copied into the kernel arguments.  Entry i is evaluated with qpos[q_adr[k]] = q[i][k], k < ncol, and everything else - the other
 * joints, the props - taken from env env_index[i].  Both NULL: the env's own qpos (ncol is ignored).  Joint equalities (the coupled fingers) are not
 * enforced: the caller gives the configuration it means.  A NaN in q makes every geom it moves unreachable (flags 4 where only such geoms are
 * asked for).  Nothing bound is ever written.  env_index may repeat an env: K waypoints against one env in one call.  An entry's output bits depend on
 * its env's state, q[i], q_adr, its pair and max_dist only.  Asynchronous on `hip_stream`.  An addition: the ABI number stays.
 *
 * SO101_ERR_ARG with the messages of so101_proximity under the name so101_tree_proximity (ngeom is the handle's, dims[4]), and: q without q_adr or
 * q_adr without q; ncol outside 1 .. 16; a q_adr entry that is not the qpos address of a hinge or slide joint; a repeated q_adr entry.
 * SO101_ERR_STATE: no state bound. */
int so101_tree_proximity(so101_tree* sim, const int32_t* env_index, int n, const float* q /* DEVICE [n][ncol] or NULL */,
                         const int32_t* q_adr /* HOST [ncol] or NULL */, int ncol,
                         const so101_tree_geom_pair* pairs /* HOST, npair of them */, int npair, float max_dist,
                         const so101_proximity_out* out, void* hip_stream);
const char* so101_tree_last_error(const so101_tree* sim);

#ifdef __cplusplus
}
#endif
#endif /* SO101_H_ */
