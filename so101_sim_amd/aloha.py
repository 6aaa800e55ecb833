"""ALOHA hand-over tasks (`HandOverBanana`, `HandOverPen`) on the general-tree engine.

Host-side mirror of the reference's `HandOver` task (so101_sim/tasks/hand_over.py:122-349) on `AlohaTask`
(so101_sim/tasks/base/aloha2_task.py:145-444) behind the same dm_env-style surface as the SO100 environments of env.py:
    env.reset() -> TimeStep    env.step(action[14]) -> TimeStep    env.action_spec()    env.observation_spec()
    env.task.get_instruction()    env.close()
Every number comes from the kernels behind the `so101_tree_*` entry points of include/so101.h (csrc/so101_tree.hpp); torch is the
array container.  n_envs == 1 yields numpy observations without the env dimension (what a caller of the reference sees), n_envs > 1
torch tensors on the GPU with a leading env dimension.

Cameras: `render_depth` casts the scene's six cameras (cameras.ALOHA_CAMERAS) or any cameras.Camera against the collision geometry
on the GPU (so101_tree_render) - depth and geom ids, from the current or the delayed state; not wired into the observation.
`render_color` (so101_tree_render_color, appearance.py) adds a colour image and surface normals of the same collision geometry,
flat-coloured per geom and Lambert-shaded by directional lights - not MuJoCo's renderer: no textures, shadows, specular term,
visual-only meshes or positional lights.
Cartesian tool control: `tool_pose`, `tool_chain`, `solve_ik` and `cartesian_action` give the pose and Jacobian of the six tool sites
(tools.ALOHA_TOOLS) or any tools.Tool and the joint values that bring one to a target, batched on the GPU (so101_tree_tool_pose / so101_tree_tool_ik).
Contact sensing: `contacts`, `touch` and `geom_group` give the contact list of the current state (64 contacts per env in the hand-over scenes, 160 in
Dining) and "who touches whom" over pairs of geom groups (contacts.aloha_groups), batched on the GPU (so101_tree_contacts).
Proximity sensing: `proximity` gives the smallest signed distance, the closest points and the normal over the same pairs of geom groups while they
do not touch - per env, or per waypoint `q` of named joints (a tool's chain: what `solve_ik` returns) against an env's props (so101_tree_proximity).
Not built: a non-default table height offset (the committed model blob is compiled for the reference's default).  The observation delays ARE parameters (`joints_observation_delay_secs`, `image_observation_delay_secs`,
aloha2_task.py:153-159: whole control steps, handed to the kernels by so101_tree_configure_env), and `physics_state` /
`delayed_physics_state` come from a device-side delay line (so101_tree_bind_physics_state).  Both reward modes are built: the overlap boxes (default) and the contact sequence
(`reward_based_on_overlap=False`, hand_over.py:286-338, with `reward_requires_handover`).
"""
from __future__ import annotations

import collections

import numpy as np

from . import native
from ._dmenv import Array, BoundedArray, TimeStep
from .model import scenes
from . import appearance as _appearance
from . import contacts as _contacts
from ._env_base import DEFAULT_CONTROL_TIMESTEP, PHYSICS_TIMESTEP, SETTLE_WARNING, EnvironmentBase, generator_of, pop_task_keywords

DEFAULT_JOINTS_DELAY_SECS, DEFAULT_PHYSICS_DELAY_SECS = 0.1, 0.3          # aloha2_task.py:102-103
NPOS, NVEL = 14, 16

# obs row of so101_tree_step (include/so101.h): joints_pos | joints_vel | undelayed_joints_pos | undelayed_joints_vel | commanded_joints_pos
_SLICES = dict(joints_pos=(0, 14), joints_vel=(14, 30), undelayed_joints_pos=(30, 44), undelayed_joints_vel=(44, 60),
               commanded_joints_pos=(60, 74))


class HandOverTask:
    """Host-side description of `HandOver` (hand_over.py:128-236)."""

    def __init__(self, object_name, reward_based_on_overlap=True, reward_requires_handover=False, **kwargs):
        if object_name not in scenes.HANDOVER_CONFIGS:
            raise ValueError(f"Invalid object name: {object_name}, must be one of {scenes.HANDOVER_CONFIGS.keys()}")
        self.object_name = object_name
        self.reward_based_on_overlap = bool(reward_based_on_overlap)         # False: the contact sequence of hand_over.py:286-338
        self.reward_requires_handover = bool(reward_requires_handover)       # (read by the contact-sequence mode only, as in the reference)
        self._pop_keywords(kwargs)
        self._instruction = scenes.ALOHA_INSTRUCTIONS[object_name]

    scene = "hand_over"

    def _pop_keywords(self, kwargs):
        """the keywords of AlohaTask (aloha2_task.py:145-160), shared by the tasks on it"""
        pop_task_keywords(self, kwargs)
        self.waist_joint_limit = float(kwargs.pop("waist_joint_limit", np.pi / 2))
        if float(kwargs.pop("table_height_offset", scenes.ALOHA_TABLE_HEIGHT_OFFSET)) != scenes.ALOHA_TABLE_HEIGHT_OFFSET:
            raise NotImplementedError("the model blob is compiled for table_height_offset = 0.011 (aloha2_task.py:107)")
        # observation delays (aloha2_task.py:153-159,236-251): dm_control delays an observable by delay_secs / physics_timestep
        # substeps; the kernels keep one sample per control step, so a delay must be a whole number of control steps (0 = undelayed)
        self.joints_observation_delay_secs = float(kwargs.pop("joints_observation_delay_secs", DEFAULT_JOINTS_DELAY_SECS))
        self.image_observation_delay_secs = float(kwargs.pop("image_observation_delay_secs", DEFAULT_PHYSICS_DELAY_SECS))
        self.joints_delay_steps = self._delay_steps(self.joints_observation_delay_secs, "joints_observation_delay_secs")
        self.physics_delay_steps = self._delay_steps(self.image_observation_delay_secs, "image_observation_delay_secs")

    def load_blob(self, real: str):
        return scenes.load_aloha_blob(self.object_name, real)

    @property
    def reward_mode(self) -> int:          # so101_tree_config.reward_mode
        return 0 if self.reward_based_on_overlap else 1

    def _delay_steps(self, secs: float, name: str) -> int:
        steps = secs / self.control_timestep
        if secs < 0 or abs(steps - round(steps)) > 1e-9 or round(steps) > 64:
            raise ValueError(f"{name} = {secs}: must be a whole number (0..64) of control steps of {self.control_timestep} s")
        return int(round(steps))

    def get_instruction(self):
        return self._instruction


class DiningPlaceInContainerTask(HandOverTask):
    """Host-side description of `DiningPlaceInContainer` (tasks/dining_place_in_container.py:26-160) on the `Dining` scene
    (tasks/base/dining.py:39-267): the ALOHA robot and six free props (mug, pen, banana, plate, bowl, container); `task_id` names the
    object / receptacle pair and its reward - 'banana' (into the bowl) and 'pen' (into the white cup): overlap boxes; 'mug' (onto the
    plate): the mug touches the plate while neither moves."""

    scene = "dining"

    def __init__(self, task_id: str = "banana", **kwargs):
        if task_id not in scenes.DINING_TASKS:
            raise ValueError(f"Unknown task ID: {task_id}")                    # dining_place_in_container.py:83-84
        cfg = scenes.DINING_TASKS[task_id]
        self.task_id = task_id
        self.object_name = cfg["object"]
        self.receptacle_name = cfg["receptacle"]
        self.reward_type = cfg["reward"]
        self.reward_based_on_overlap = cfg["reward"] == "bbox"
        self.reward_requires_handover = False
        self._pop_keywords(kwargs)
        self._instruction = cfg["instruction"]

    def load_blob(self, real: str):
        return scenes.load_dining_blob(self.task_id, real)

    @property
    def reward_mode(self) -> int:
        return scenes.DINING_REWARD_MODE[self.reward_type]


def aloha_action_spec(ctrlrange: np.ndarray, waist_joint_limit: float = np.pi / 2) -> BoundedArray:
    """AlohaTask.action_spec (aloha2_task.py:279-301): the actuators' ctrlrange, waists cut to +-waist_joint_limit, grippers in
    follower units; shape (14,), float32."""
    lo, hi = ctrlrange[:, 0].astype(np.float32), ctrlrange[:, 1].astype(np.float32)
    lo[0] = lo[7] = -waist_joint_limit
    hi[0] = hi[7] = waist_joint_limit
    lo[6] = lo[13] = scenes.ALOHA_GRIPPER_LIMITS["follower"][1]
    hi[6] = hi[13] = scenes.ALOHA_GRIPPER_LIMITS["follower"][0]
    return BoundedArray((14,), np.float32, lo, hi)


class AlohaEnvironment(EnvironmentBase):
    def __init__(self, task: HandOverTask, n_envs: int = 1, time_limit: float = float("inf"), random_state=None, device=None,
                 env_id_base: int = 0, solver_iterations: int = 0, solver_tolerance: float = -1.0, settle_max_substeps: int = 1000,
                 physics_state: bool | None = None, seed_compatible: bool = True, narrowphase: str = "epa", prefetch_resets: bool = True, pipeline: bool = True):
        # N = 1: the reference's placements come from np.random.RandomState(seed) inside dm_control's PropPlacers.  With
        # seed_compatible (default) a single env draws them from the same generator in the same order - object position (3 draws,
        # hand_over.py:36-40), object yaw (1, :41-49), container position (3 per attempt, <= 20 attempts against collisions, :51-56) -
        # and lets the kernels settle (so101_tree_settle).  Batches key the kernels' counter RNG by (seed, env id, episode) instead.
        self._seed_compatible = bool(seed_compatible) and int(n_envs) == 1
        self._np_random = generator_of(random_state)
        self._pending_first = False
        self._open_device(task, n_envs, device, random_state, host_draws=self._seed_compatible)
        torch, seed, N = self.torch, self.seed, self.n_envs
        blob, self.meta = task.load_blob("f32")
        m, m64 = self._model(), self._model("f64")      # (f64: the distributions' bounds unrounded: the draws must be the reference's, bit for bit)
        self._ctrlrange = np.asarray(m["act_ctrlrange"], dtype=np.float64).reshape(-1, 2)
        qadr = np.asarray(m["body_qposadr"])
        if task.scene == "dining":
            self._dining = dict(lo=np.asarray(m64["task_region_lo"], dtype=np.float64).reshape(6, 3), hi=np.asarray(m64["task_region_hi"], dtype=np.float64).reshape(6, 3),
                                qadr=[int(qadr[b]) for b in np.asarray(m["task_prop_bodies"]).ravel()])
        self._placer = dict(self._hand_over_placer(), qo=int(qadr[int(np.asarray(m["task_object_body"]).ravel()[0])]),
                            qc=int(qadr[int(np.asarray(m["task_container_body"]).ravel()[0])]))
        with torch.cuda.device(self.device):
            # "mpr": the -DSO101_MPR build of the library, built on demand
            self.sim = native.TreeSim(blob, N, device=self.device.index or 0, lib_path=self._narrowphase_library(narrowphase))
        s = self.sim
        if (s.nu, s.obs_dim) != (NPOS, 3 * NPOS + 2 * NVEL):
            raise RuntimeError("unexpected model dimensions for an ALOHA scene")
        z = self._zeros
        self.qpos, self.qvel, self.ctrl, self.warm = z(s.nq, N), z(s.nv, N), z(s.nu, N), z(s.nv, N)
        jd, pd = task.joints_delay_steps, task.physics_delay_steps
        self._ring_pos, self._ring_vel = z(max(jd, 1), NPOS, N), z(max(jd, 1), NVEL, N)
        self.ep_return, self.step_count, self.episode = z(N), z(N, dt=torch.int32), z(N, dt=torch.int32)
        self.obs, self.reward, self.discount = z(N, s.obs_dim), z(N), z(N)
        self.step_type = z(N, dt=torch.uint8)
        self._action = z(N, s.nu)
        self._diag = z(N, 8, dt=torch.int32)
        s.bind(*(t.data_ptr() for t in (self.qpos, self.qvel, self.ctrl, self.warm)))
        s.bind_env(*(t.data_ptr() for t in (self._ring_pos, self._ring_vel, self.ep_return, self.step_count, self.episode)))
        nsub = int(round(task.control_timestep / PHYSICS_TIMESTEP))
        self.last_step = scenes.time_limit_last_step(time_limit, task.control_timestep, PHYSICS_TIMESTEP) if np.isfinite(time_limit) else 1 << 30
        s.configure_env(n_substeps=nsub, last_step=self.last_step, settle_max_substeps=int(settle_max_substeps),
                        terminate_on_success=int(task.terminate_episode), solver_iterations=int(solver_iterations),
                        solver_tolerance=float(solver_tolerance), seed=seed, env_id_base=int(env_id_base),
                        reward_mode=task.reward_mode, reward_requires_handover=int(task.reward_requires_handover),
                        joints_delay_steps=jd, physics_delay_steps=pd,
                        # reset prefetch (batches; a seed-compatible single env draws its placements on the host: nothing to settle ahead)
                        prefetch_resets=int(bool(prefetch_resets) and not self._seed_compatible),
                        # the step as a launch chain (narrowphase in a launch of its own; the contact rewards end the chain with one more narrowphase
                        # launch on the post-step state + k_tree_pipe_finish); one env is one wavefront either way and keeps the single launch
                        pipeline=int(bool(pipeline) and self.n_envs > 1))
        self._pipeline = bool(pipeline)
        # physics_state / delayed_physics_state (aloha2_task.py:244-251,441-444): qpos | qvel and its copy of `pd` control steps ago,
        # from a device-side delay line the step / reset kernels maintain.  The reference ties them to image_observation_enabled;
        # for batches they are opt-in (58 + 58 floats per env and step).
        self._with_state = bool(task.image_observation_enabled if physics_state is None and N == 1 else physics_state)
        self._ps_dim = s.nq + s.nv
        if self._with_state:
            self._bind_physics_state(max(pd, 1), self._ps_dim)

    # ------------------------------------------------------------------ specs
    def action_spec(self) -> BoundedArray:
        return aloha_action_spec(self._ctrlrange, self.task.waist_joint_limit)

    def observation_spec(self):
        spec = collections.OrderedDict()
        spec["commanded_joints_pos"] = Array((NPOS,), np.float64, "commanded_joints_pos")
        spec["joints_pos"] = Array((NPOS,), np.float64, "joints_pos")
        spec["joints_vel"] = Array((NVEL,), np.float64, "joints_vel")
        if self._with_state:
            spec["physics_state"] = Array((self._ps_dim,), np.float64, "physics_state")
        if self.task.joints_delay_steps:          # (the undelayed_* / delayed_* copies exist only with a joints delay, aloha2_task.py:236-243)
            spec["undelayed_joints_pos"] = Array((NPOS,), np.float64, "undelayed_joints_pos")
            spec["undelayed_joints_vel"] = Array((NVEL,), np.float64, "undelayed_joints_vel")
            spec["delayed_joints_pos"] = Array((NPOS,), np.float64, "delayed_joints_pos")
            spec["delayed_joints_vel"] = Array((NVEL,), np.float64, "delayed_joints_vel")
        if self._with_state and self.task.physics_delay_steps:
            spec["delayed_physics_state"] = Array((self._ps_dim,), np.float64, "delayed_physics_state")
        return spec

    def _load_blob(self, real: str):
        return self.task.load_blob(real)

    def _debug_layout(self):
        return self.sim.dbg, self.sim.debug_dim

    # ------------------------------------------------------------------ stepping
    def _obs_dict(self):
        o = collections.OrderedDict()
        cut = lambda k: self.obs[:, _SLICES[k][0]:_SLICES[k][1]]
        o["commanded_joints_pos"] = cut("commanded_joints_pos")
        o["joints_pos"] = cut("joints_pos")
        o["joints_vel"] = cut("joints_vel")
        if self._with_state:
            o["physics_state"] = self.physics_state
        if self.task.joints_delay_steps:
            o["undelayed_joints_pos"] = cut("undelayed_joints_pos")
            o["undelayed_joints_vel"] = cut("undelayed_joints_vel")
            o["delayed_joints_pos"] = cut("joints_pos")
            o["delayed_joints_vel"] = cut("joints_vel")
        if self._with_state and self.task.physics_delay_steps:
            o["delayed_physics_state"] = self.delayed_physics_state
        if self.n_envs == 1:
            return collections.OrderedDict((k, v[0].double().cpu().numpy()) for k, v in o.items())
        return o

    def step_tensor(self, action):
        """action: float tensor [N, 14] on the device.  Fills and returns (obs, reward, discount, step_type)."""
        if tuple(action.shape) != (self.n_envs, NPOS):
            raise ValueError(f"Expected 14 joint positions per env, got {tuple(action.shape)}")
        self._action.copy_(action)
        self.sim.step(self._action.data_ptr(), self.obs.data_ptr(), self.reward.data_ptr(), self.discount.data_ptr(),
                      self.step_type.data_ptr(), self._stream())
        return self.obs, self.reward, self.discount, self.step_type

    def _timestep(self):
        obs = self._obs_dict()
        if self.n_envs == 1:
            st = int(self.step_type[0])
            if st == 0:
                return TimeStep(st, None, None, obs)
            return TimeStep(st, float(self.reward[0]), float(self.discount[0]), obs)
        return TimeStep(self.step_type, self.reward, self.discount, obs)

    def _reset_seed_compatible_dining(self):
        """Dining._sample_props + the two PropPlacers (dining.py:162-267) with numpy's generator, in the reference's order: six region
        samples `uniform(low, high)` (top left / middle / right, bottom left / middle / right: three numbers each), `shuffle` of the top and
        of the bottom ordering, then per prop in the order plate, bowl, container, mug, pen, banana one `uniform(-pi, pi)` yaw (positions
        come from a deterministic Sequence); collisions ignored; settle and episode start by the kernels."""
        torch, D, rs, s = self.torch, self._dining, self._np_random, self.sim
        samples = [rs.uniform(low=D["lo"][r], high=D["hi"][r]) for r in range(6)]
        top, bottom = [0, 1, 2], [3, 4, 5]
        rs.shuffle(top)
        rs.shuffle(bottom)
        regions = [top[0], top[1], top[2], bottom[0], bottom[1], bottom[2]]          # plate, bowl, container, mug, pen, banana
        q = np.zeros(s.nq)
        q[:16] = np.concatenate([scenes.ALOHA_HOME_QPOS, scenes.ALOHA_HOME_QPOS])
        yaws = []
        for p in range(6):
            yaw = rs.uniform(-np.pi, np.pi)
            a = D["qadr"][p]
            q[a:a + 3] = samples[regions[p]]
            q[a + 3:a + 7] = [np.cos(0.5 * yaw), 0.0, 0.0, np.sin(0.5 * yaw)]
            yaws.append(float(yaw))
        self.ctrl.copy_(torch.as_tensor(np.concatenate([scenes.ALOHA_HOME_CTRL, scenes.ALOHA_HOME_CTRL]), dtype=torch.float32, device=self.device).unsqueeze(1))
        self._write_state(q)
        self.placements = dict(zip(scenes.DINING_PLACER_ORDER, [dict(position=samples[regions[p]].copy(), yaw=yaws[p], region=int(regions[p])) for p in range(6)]))
        s.settle(self._stream())
        s.begin_episode(self._stream())
        self.episode += 1
        if int(self.diagnostics()[0, 4]) & 32:
            import warnings
            warnings.warn(SETTLE_WARNING)

    def _reset_seed_compatible(self):
        """placements from numpy's generator in dm_control's PropPlacer order, settle and episode start by the kernels"""
        if self.task.scene == "dining":
            return self._reset_seed_compatible_dining()
        torch, P, s = self.torch, self._placer, self.sim
        q = np.zeros(s.nq)
        q[:16] = np.concatenate([scenes.ALOHA_HOME_QPOS, scenes.ALOHA_HOME_QPOS])           # aloha2_task.py:374-377
        self.ctrl.copy_(torch.as_tensor(np.concatenate([scenes.ALOHA_HOME_CTRL, scenes.ALOHA_HOME_CTRL]), dtype=torch.float32, device=self.device).unsqueeze(1))
        self._place_hand_over(q, P["qo"], P["qc"])
        s.settle(self._stream())
        s.begin_episode(self._stream())
        self.episode += 1
        if int(self.diagnostics()[0, 4]) & 32:
            import warnings
            warnings.warn(SETTLE_WARNING)

    def reset(self) -> TimeStep:
        """every env starts a new episode; returns FIRST"""
        if self._seed_compatible:
            self._reset_seed_compatible()
        else:
            self.sim.reset(None, self._stream())
        self._pending_first = False
        self.torch.cuda.current_stream(self.device).synchronize()
        # the FIRST observation is written by the step kernel for an env that resets inside a step call; for an explicit reset it
        # is assembled here from the state the reset left
        q = self.qpos.t()
        pos = q[:, [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14]].clone()
        (qo, qc), (_, _), (fo, fc) = scenes.ALOHA_GRIPPER_LIMITS["sim_qpos"], scenes.ALOHA_GRIPPER_LIMITS["sim_ctrl"], scenes.ALOHA_GRIPPER_LIMITS["follower"]
        for k in (6, 13):
            pos[:, k] = (pos[:, k] - qc) / (qo - qc) * (fo - fc) + fc
        cmd = self.ctrl.t().clone()
        (co, cc) = scenes.ALOHA_GRIPPER_LIMITS["sim_ctrl"]
        for k in (6, 13):
            cmd[:, k] = (cmd[:, k] - cc) / (co - cc) * (fo - fc) + fc
        vel = self.qvel.t()[:, :NVEL]
        self.obs[:, 0:14], self.obs[:, 14:30], self.obs[:, 30:44], self.obs[:, 44:60], self.obs[:, 60:74] = pos, vel, pos, vel, cmd
        self.step_type.zero_(); self.reward.zero_(); self.discount.fill_(1.0)
        ts = self._timestep()
        return TimeStep(ts.step_type, None, None, ts.observation)       # FIRST carries no reward / discount

    def step(self, action) -> TimeStep:
        torch = self.torch
        a = torch.as_tensor(np.asarray(action) if not torch.is_tensor(action) else action, dtype=torch.float32, device=self.device)
        if a.dim() == 1:
            a = a.unsqueeze(0)
        if self._pending_first:                # the step after LAST restarts the episode and reports FIRST (dm_control); the host draws
            return self.reset()                # the next placements, the kernels' own auto-reset is not used
        self.step_tensor(a)
        if self._seed_compatible and int(self.step_type[0]) == 2:
            self._pending_first = True
        return self._timestep()

    def compute_settled(self, n_episodes: int, first_episode: int = 0):
        """Placement + settle of the first episodes of every env, done once at the width of the machine (one launch per episode) and
        attached: the resets of those episodes - explicit or inside step calls - become copies, bit-identical to settling in place.
        Batches only (a seed-compatible single env draws its placements on the host)."""
        if self._seed_compatible:
            raise RuntimeError("a seed-compatible single env draws its placements from numpy's generator; nothing to precompute")
        torch, s, N = self.torch, self.sim, self.n_envs
        z = self._zeros
        self._store = (z(n_episodes, s.nq, N), z(n_episodes, s.nv, N), z(n_episodes, s.nv, N), z(n_episodes, N, dt=torch.int32))
        s.compute_settled(first_episode, n_episodes, *(t.data_ptr() for t in self._store), self._stream())
        self.torch.cuda.current_stream(self.device).synchronize()
        s.set_settled_store(first_episode, n_episodes, *(t.data_ptr() for t in self._store))
        return self._store

    # ------------------------------------------------------------------ depth / segmentation cameras (cameras.py)
    def render_depth(self, camera, height: int, width: int, env_ids=None, segmentation: bool = True, delayed: bool = False):
        """Depth and geom-id images of the collision geometry, by ray casting on the GPU (so101_tree_render).

        camera: a name of cameras.ALOHA_CAMERAS, a cameras.Camera (its `body` a body id or a name of `meta["body_names"]`), or a
        sequence of either (at most 8).
        env_ids: env indices to render (sequence or tensor), None = all.
        delayed: False renders the current state, True the state of `image_observation_delay_secs` ago - the qpos of
        `delayed_physics_state`, what the reference's delayed camera observables show; it needs the env's physics-state line
        (`physics_state=True` for batches).
        Returns (depth [n, ncam, height, width] float32, seg int32 of the same shape or None) on the env's device, for any n_envs.
        depth is the distance along the optical axis, +inf where the ray hits nothing; seg the geom index
        (`meta["geom_names"][i]` names it), -1 where it hits nothing.  This is not RGB: textures and visual-only meshes are not
        rendered, and a camera's horizontal extent follows from square pixels."""
        from . import cameras as _cameras
        cams = [c.with_body_ids(self.meta["body_names"]) for c in _cameras.resolve(camera, _cameras.ALOHA_CAMERAS)]
        if delayed and not self._with_state:
            raise ValueError("render_depth(delayed=True) needs the physics-state delay line: create the environment with physics_state=True")
        return self._render_depth(cams, height, width, env_ids, segmentation, source=1 if delayed else 0)

    # ------------------------------------------------------------------ colour cameras (appearance.py: ColorCameras)
    _scene_shading = _appearance.ALOHA_SHADING

    def _scene_colors(self):
        return _appearance.aloha_colors(self.meta)

    def render_color(self, camera, height: int, width: int, env_ids=None, colors=None, shading=None, normals: bool = False, depth: bool = False,
                     segmentation: bool = False, delayed: bool = False):
        """Colour images of the collision geometry, by ray casting and shading on the GPU (so101_tree_render_color).

        camera, env_ids, delayed: as in render_depth.  colors: None (the scene's table, appearance.aloha_colors), a float32 [ngeom, 3]
        array or tensor, [n_envs, ngeom, 3] for colours per env (the rendered env's row is used), or a dict {anything geom_group()
        takes: rgb} applied over the scene's table.  shading: an appearance.Shading, None = appearance.ALOHA_SHADING.
        Returns appearance.ColorImages(rgb, normal, depth, seg) on the env's device: rgb uint8 [n, ncam, height, width, 3]; with
        normals=True the world-frame unit surface normal float32 [n, ncam, height, width, 3] (0 where the ray hits nothing); with
        depth / segmentation what render_depth returns, bit for bit; None otherwise.  This is not MuJoCo's renderer: what is drawn is
        the collision geometry of render_depth, flat-coloured per geom and Lambert-shaded by directional lights - no textures, shadows,
        specular term, visual-only meshes or positional lights."""
        from . import cameras as _cameras
        cams = [c.with_body_ids(self.meta["body_names"]) for c in _cameras.resolve(camera, _cameras.ALOHA_CAMERAS)]
        if delayed and not self._with_state:
            raise ValueError("render_color(delayed=True) needs the physics-state delay line: create the environment with physics_state=True")
        return self._render_color(cams, height, width, env_ids, colors, shading, normals, depth, segmentation, source=1 if delayed else 0)

    # ------------------------------------------------------------------ Cartesian tool control (tools.py)
    def _resolve_tool(self, tool):
        from . import tools as _tools
        return _tools.resolve(tool, _tools.ALOHA_TOOLS).with_body_ids(self.meta["body_names"])

    def _tool_columns(self, t):
        return len(self.sim.tool_chain(t.body)[0])

    def _ik_config(self, t, mode, config):
        lo, hi = self.ik_limits(t)
        return self.sim.ik_config(t.body, **dict(dict(q_lo=lo, q_hi=hi), mode=mode, **config))

    def tool_chain(self, tool="left/gripper"):
        """The joints a tool depends on, root first: (dof indices into qvel, qpos addresses, joint types - native.TREE_JNT_HINGE / TREE_JNT_SLIDE).
        They are the columns of tool_pose's Jacobian and of solve_ik's q."""
        return self.sim.tool_chain(self._resolve_tool(tool).body)

    def tool_pose(self, tool="left/gripper", env_ids=None, q=None, jacobian: bool = False):
        """World pose of a tool frame (tools.Tool or a name of tools.ALOHA_TOOLS) on the GPU (so101_tree_tool_pose): at the current qpos of the
        envs `env_ids` (None = all), or at explicit joint values `q` [n, ncol] of the tool's chain (tool_chain).  Returns (pos [n, 3],
        mat [n, 3, 3]) and, with jacobian=True, jac [n, 6, ncol] - rows 0-2 the translational, rows 3-5 the rotational Jacobian of MuJoCo's
        mj_jacSite, column k for dof tool_chain(tool)[0][k]."""
        return self._tool_pose(tool, env_ids, q, jacobian)

    def ik_limits(self, tool="left/gripper"):
        """Default joint limits of solve_ik for a tool, (lo [ncol], hi [ncol]) float64: the model's jnt_range of the chain's joints, intersected
        with action_spec() on the actuated arm joints - so the waist stays within the task's waist_joint_limit."""
        t = self._resolve_tool(tool)
        dof, _, _ = self.sim.tool_chain(t.body)
        cfg = self.sim.ik_config(t.body)
        lo, hi = np.array(cfg.q_lo[:len(dof)], dtype=np.float64), np.array(cfg.q_hi[:len(dof)], dtype=np.float64)
        spec, cols = self.action_spec(), self._action_columns()
        for k, d in enumerate(dof):
            a = cols.get(d)
            if a is not None:
                lo[k], hi[k] = max(lo[k], float(spec.minimum[a])), min(hi[k], float(spec.maximum[a]))
        return lo, hi

    def _action_columns(self):
        """dof -> action column of the actuated arm joints (the grippers' entries are in follower units, not joint values: left out)"""
        if getattr(self, "_act_cols", None) is None:
            m = self._model()
            grip = np.asarray(m["task_act_is_gripper"]).ravel()
            self._act_cols = {int(d): a for a, d in enumerate(np.asarray(m["act_dof"]).ravel()) if not int(grip[a])}
            self._grip_cols = [a for a in range(len(grip)) if int(grip[a])]
        return self._act_cols

    def solve_ik(self, target_pos, target_mat=None, tool="left/gripper", mode=None, q_init=None, env_ids=None, **config):
        """Joint values that bring a tool to Cartesian targets, one damped least-squares solve per row on the GPU (so101_tree_tool_ik).

        target_pos [n, 3]; target_mat [n, 3, 3] or None.  mode: 0 position only, 1 position and the direction of the tool's z axis,
        2 position and full orientation; None = 0 without target_mat, else 1.  q_init [n, ncol] (the tool's chain, tool_chain) starts
        the solves; None starts them from the current qpos of the envs `env_ids` (None = envs 0 .. n - 1).  **config replaces fields of
        the default settings (max_iters, tol_pos, tol_rot, rot_weight, damping, max_step, free_mask, q_lo, q_hi; include/so101.h
        so101_tree_ik_config); the default limits are ik_limits(tool), the default free_mask the hinge columns - a finger's slide joint is held.
        Returns (q [n, ncol], converged [n] bool, residual [n, 2] = position error in metres and orientation error in radians at q,
        iters [n] int32, -1 where not converged)."""
        return self._solve_ik(target_pos, target_mat, tool, mode, q_init, env_ids, config)

    def cartesian_action(self, left=None, right=None, gripper_left=None, gripper_right=None, mode=None, **config):
        """An [N, 14] action for step_tensor() that commands the grippers of every env to Cartesian targets.  `left` / `right`:
        (target_pos [N, 3], target_mat [N, 3, 3] or None) for the tool "left/gripper" / "right/gripper", solved from the current qpos
        (solve_ik; mode and **config go there); the solution fills that arm's six entries.  An arm without a target keeps its entries of
        commanded_joints_pos, a gripper not given (`gripper_left` / `gripper_right`: scalar or [N], the action's follower units) its
        commanded entry.  The step neither clips nor converts arm entries, so the ctrl commanded for a solved arm IS the solution, bit for
        bit.  Targets the solve does not reach still give its last iterate: check solve_ik() where that matters."""
        lo, hi = _SLICES["commanded_joints_pos"]
        action = self.obs[:, lo:hi].clone()
        cols = self._action_columns()
        for name, target in (("left/gripper", left), ("right/gripper", right)):
            if target is None:
                continue
            target_pos, target_mat = target
            q, _, _, _ = self.solve_ik(target_pos, target_mat, tool=name, mode=mode, **config)
            if q.shape[0] != self.n_envs:
                raise ValueError(f"cartesian_action needs one target per env ({self.n_envs}), got {q.shape[0]}")
            for k, d in enumerate(self.tool_chain(name)[0]):
                action[:, cols[d]] = q[:, k]
        for a, g in zip(self._grip_cols, (gripper_left, gripper_right)):
            if g is not None:
                action[:, a] = self._f32(g)
        return action

    # ------------------------------------------------------------------ contact sensing (contacts.py: ContactSensing)
    _geom_limit = _contacts.TREE_MAX_GEOMS
    _contact_capacity = property(lambda self: self.sim.max_contacts)          # (64 in the hand-over scenes, 160 in Dining)

    def _geom_groups(self):
        if getattr(self, "_groups", None) is None:
            self._groups = _contacts.aloha_groups(self.meta, self._model())
        return self._groups

    def geom_group(self, spec):
        """A contacts.GeomGroup from a group name of the scene (contacts.aloha_groups: every body name, "left_arm", "right_arm", "arms",
        "left_gripper", "right_gripper", "grippers", "object", "container", "props"), a geom name, an fnmatch pattern over the geom names, an
        iterable of geom ids or a GeomGroup.  ALOHA geom names are not unique (`vx300s_8_custom_finger_left` occurs once per arm): a geom
        name or a pattern resolves to ALL geoms that match."""
        return self._geom_group(spec)

    def contacts(self, env_ids=None, forces: bool = False):
        """The contact lists of the envs `env_ids` (None = all) at their current state, on the GPU (so101_tree_contacts): a
        contacts.ContactReport of tensors on the env's device - count [n], flags [n] (1 candidate overflow, 2 contact overflow: the list ends at
        the first geom pair that does not fit the C contacts, 4 with forces: the rows of the last contacts did not fit, they report zero force),
        geom [n, C, 2], dist [n, C], pos [n, C, 3], frame [n, C, 3, 3] (rows: normal geom1 -> geom2 and two tangents, MuJoCo's contact.frame) and,
        with forces=True, force [n, C, 6] (mj_contactForce), else None; C = 64 in the hand-over scenes, 160 in Dining (`sim.max_contacts`).
        Slots beyond count hold geoms -1, dist +inf, zeros.  The forces are those of a forward pass at the current state (constraint rows and
        solve, warmstart read and left alone), not the impulses of the last substep; without forces only kinematics and collision run.
        There is no `physics` facade on this environment: `contacts.records(report, entry)` gives the list of `physics.data.contact`-like
        records of one entry."""
        return self._contacts(env_ids, forces)

    def touch(self, pairs, env_ids=None, forces: bool = False):
        """Who touches whom: `pairs` is a sequence of at most 16 (a, b), each side anything geom_group() takes.  Per env of `env_ids` (None = all)
        and pair, reduced on the GPU from the env's contact list: a contacts.TouchReport of count [n, npair] int32 (contacts with one geom in a
        and the other in b), touching = count > 0, dist [n, npair] (the smallest, +inf without a contact) and, with forces=True,
        normal_force [n, npair] (sum of the normal forces) and force [n, npair, 3] (the net world-frame force ON group a), else None.
        `("right_gripper", "object")`, `("left_gripper", "object")` and `("object", "container")` are the questions of the contact-sequence
        reward (hand_over.py:286-338), the last one that of the Dining `contact` reward."""
        return self._touch(pairs, env_ids, forces)

    # ------------------------------------------------------------------ proximity sensing (proximity.py: ProximitySensing)
    _q_is_columns = True

    def _proximity_columns(self, joints):
        """qpos addresses of q's columns: a tool's chain, explicit addresses, or (None) all one-dof joints in qpos order"""
        from . import tools as _tools
        if joints is None:
            if getattr(self, "_onedof_qadr", None) is None:
                m = self._model()
                jt, qadr = np.asarray(m["body_jnttype"]).ravel(), np.asarray(m["body_qposadr"]).ravel()
                self._onedof_qadr = sorted(int(qadr[b]) for b in range(len(jt)) if int(jt[b]) in (native.TREE_JNT_HINGE, native.TREE_JNT_SLIDE))
            return list(self._onedof_qadr)
        if isinstance(joints, (str, _tools.Tool)):
            return [int(a) for a in self.sim.tool_chain(self._resolve_tool(joints).body)[1]]
        try:
            adr = [int(a) for a in joints]
        except (TypeError, ValueError):
            raise ValueError(f"joints must be a tool, a tool name or a sequence of qpos addresses, got {joints!r}") from None
        if not 1 <= len(adr) <= 16 or len(set(adr)) != len(adr):
            raise ValueError(f"joints must name 1 .. 16 distinct qpos addresses, got {adr}")
        return adr

    def proximity(self, pairs, env_ids=None, q=None, joints=None, max_dist: float = 0.1):
        """How far apart: `pairs` is a sequence of 1 to 16 (a, b), each side anything geom_group() takes.  Per entry and pair, on the GPU
        (so101_tree_proximity), a proximity.ProximityReport of tensors on the env's device: dist [n, P], geom [n, P, 2] int32,
        point [n, P, 2, 3], normal [n, P, 3], flags [n, P] int32 - the report, the conventions and the flag bits of
        BatchedEnvironment.proximity (1 penetrating, 2 iteration cap, 4 nothing within max_dist, 8 env id out of range).

        Entries: the envs `env_ids` (None = all; an env may repeat).  With `q` [n, ncol], entry i is evaluated with the joints `joints` at
        q[i] and everything else - the other arm, the props - where env env_ids[i] has it; env_ids = [e] * K checks K waypoints against one
        env in one call.  `joints`: a tool name or tools.Tool - q's columns are that tool's chain (tool_chain), so q is exactly what
        solve_ik(tool=...) returned: 6 columns for a gripper, 7 for a finger; or a sequence of 1 .. 16 qpos addresses of hinge or slide
        joints; or None: all one-dof joints in qpos order, q [n, 16].  Joint equalities (the coupled fingers) are not enforced: q is the
        configuration the caller means.  A prop cannot be moved through q.  Nothing bound is modified.

        `dist` is the smallest signed distance over the geom pairs (one geom in a, the other in b) the model's pair list admits - the list the
        collision stage walks, so "proximity < 0" and touch() speak about the same pairs.  Separated: the Euclidean gap, >= 0.  Penetrating:
        the smallest contact dist of the narrowphase for that geom pair, bit for bit touch()'s dist, flags bit 1.  Nothing below `max_dist`
        (finite, above 0, at most 10 m): dist = max_dist, geom -1, zeros, flags bit 4."""
        return self._proximity(pairs, env_ids, q, max_dist, joints=joints)

    def episode_returns(self):
        return self.ep_return

    def launch_plan(self) -> dict:
        """What the last `step_tensor` call enqueued, as the LIBRARY counted it (`so101_tree_last_plan`; round 5 re-implemented the slicing rule
        of csrc/tu_tree.hip here, which a change over there or a late SO101_TREE_SLICES would silently falsify - ADVICE r5).  Launch chain:
        per env slice one memset, k_tree_pipe_begin, n_substeps x (k_tree_narrow + k_tree_pipe_solve), and for the contact rewards one more
        k_tree_narrow + k_tree_pipe_finish."""
        slices, launches, memsets, path = self.sim.last_plan()
        if path == 0:
            return {"path": "no step yet", "slices": 0, "kernel_launches": 0, "memsets": 0}
        if path == 1:
            return {"path": "single kernel (k_tree_step)", "slices": 1, "kernel_launches": launches, "memsets": memsets}
        nsub = int(round(self.task.control_timestep / PHYSICS_TIMESTEP))
        post = self.task.reward_mode != 0
        return {"path": "launch chain", "slices": slices, "kernel_launches": launches, "memsets": memsets,
                "kernels": "k_tree_pipe_begin + %d x (k_tree_narrow + k_tree_pipe_solve)%s per slice" % (nsub, " + k_tree_narrow + k_tree_pipe_finish" if post else "")}

    def diagnostics(self):
        """per env: contacts, constraint rows, solver iterations, broadphase candidates, flags of the last substep"""
        self.sim.get_diag(self._diag.data_ptr(), self._stream())
        return self._diag
