"""Batched dm_env-style environment over the HIP step library.

Mirrors the surface callers of the reference use:
    env.reset() -> TimeStep         env.step(action) -> TimeStep        env.action_spec()
    env.observation_spec()          env.close()         env.task.get_instruction()     env.physics
`composer.Environment` semantics kept: FIRST has reward/discount None; a step after LAST resets and
returns FIRST; no bounds validation of actions; wrong action length raises ValueError
(scripts/so101_calibration.py:71-72).

N == 1 (`SingleEnvironment`, what `create_task_env` returns by default) yields numpy observations
with exactly the reference's keys and shapes; N > 1 (`BatchedEnvironment`) yields torch tensors on
the GPU with a leading env dimension.  PyTorch is only the array container: every number is produced
by the kernels behind include/so101.h.
"""
from __future__ import annotations

import collections
import hashlib

import numpy as np

from . import native
from ._dmenv import BoundedArray, Array, StepType, TimeStep
from .calibration import SO101Calibration
from .model import scenes
from . import appearance as _appearance
from . import contacts as _contacts
from ._env_base import DEFAULT_CONTROL_TIMESTEP, PHYSICS_TIMESTEP, SETTLE_WARNING, EnvironmentBase, generator_of, pop_task_keywords

_JOINT_DELAY_STEPS = 5       # 0.1 s / 0.02 s  (so100_task.py:81,196-201)
_PHYSICS_DELAY_STEPS = 15    # 0.3 s / 0.02 s  (so100_task.py:80,204-210)


def so100_action_spec(rotation_joint_limit: float = np.pi) -> BoundedArray:
    """SO100Task.action_spec (so100_task.py:232-251): ctrlrange of scene_pbr.xml:11 (+-3.14158) with
    [0] := +-rotation_joint_limit and [5] := [0, 0.08]; shape (6,), float32."""
    lo = np.full(6, -3.14158, dtype=np.float32)
    hi = np.full(6, 3.14158, dtype=np.float32)
    lo[0], hi[0] = -rotation_joint_limit, rotation_joint_limit
    lo[5], hi[5] = 0.0, 0.08
    return BoundedArray((6,), np.float32, lo, hi)


OBSERVATION_KEYS = ("commanded_joints_pos", "joints_pos", "joints_vel", "physics_state", "undelayed_joints_pos",
                    "undelayed_joints_vel", "delayed_physics_state")   # examples/so101_rl_breakdown.ipynb:65 (cameras excluded)


class SO100HandOverTask:
    """Host-side description of `SO100HandOver` (so101_sim/tasks/so100_hand_over.py:121-236)."""

    def __init__(self, object_name, reward_based_on_overlap=True, **kwargs):
        if object_name not in scenes.HANDOVER_CONFIGS:
            raise ValueError(f"Invalid object name: {object_name}, must be one of {scenes.HANDOVER_CONFIGS.keys()}")
        if not reward_based_on_overlap:
            raise NotImplementedError(
                "contact+distance reward mode (so100_hand_over.py:277-318) is not built: in the reference that branch looks up "
                "a body 'so100/hand_link' which scene_pbr.xml does not define, so it raises there as well")
        self.object_name = object_name
        pop_task_keywords(self, kwargs)
        self.rotation_joint_limit = float(kwargs.pop("rotation_joint_limit", np.pi))
        self._instruction = scenes.HANDOVER_CONFIGS[object_name]["instruction"]
        # the calibration file is looked up relative to the CWD at construction time, as in the reference
        self.calibration = SO101Calibration()

    def get_instruction(self):
        return self._instruction


class _PhysicsView:
    """Partial stand-in for `env.physics`: exposes `.data.qpos/.qvel/.ctrl` views of env 0, `.data.contact` / `.data.ncon`
    (n_envs == 1) and `.time()`; rendering is out of scope."""

    class _Data:
        """`contact` and `ncon` are computed when they are read (one so101_contacts launch and a copy of the list), at the state the env is
        in then - dm_control's physics.step ends on the position stage at the new state, so its data.contact is that list as well."""

        def __init__(self, env):
            self._env = env

        def _report(self):
            if self._env.n_envs != 1:
                raise AttributeError("physics.data.contact / ncon exist for n_envs == 1; a batch reads env.contacts() / env.touch()")
            return self._env.contacts()

        @property
        def contact(self):
            from . import contacts as _contacts
            return _contacts.records(self._report())

        @property
        def ncon(self):
            return int(self._report().count[0])

    def __init__(self, env):
        self._env = env
        self.data = self._Data(env)

    def _refresh(self):
        e = self._env
        self.data.qpos = e.qpos[:, 0].detach().cpu().numpy().astype(np.float64)
        self.data.qvel = e.qvel[:, 0].detach().cpu().numpy().astype(np.float64)
        self.data.ctrl = e.ctrl[:, 0].detach().cpu().numpy().astype(np.float64)
        return self

    def time(self):
        return float(self._env.step_count[0].item()) * self._env.task.control_timestep

    def get_state(self):
        self._refresh()
        return np.concatenate([self.data.qpos, self.data.qvel])

    def render(self, *a, **k):
        raise NotImplementedError("rendering is outside the MI355X hot path (SURVEY.md 8b)")


class BatchedEnvironment(EnvironmentBase):
    def __init__(self, task: SO100HandOverTask, n_envs: int = 1, time_limit: float = float("inf"),
                 random_state=None, device=None, env_id_base: int = 0, solver_iterations: int = 0,
                 solver_tolerance: float = -1.0, settle_max_substeps: int = 1000, solver: str = "newton",
                 prefetch_resets: bool = True, physics_state: bool = False, narrowphase: str = "epa"):
        self._open_device(task, n_envs, device, random_state)
        torch, seed = self.torch, self.seed
        blob, self.meta = self._load_blob("f32")
        with torch.cuda.device(self.device):
            # (an explicit lib_path here used to override SO101_HIP_LIB)
            lib = self._narrowphase_library(narrowphase, env_names_library=True)
            self.sim = native.Sim(blob, self.n_envs, device=self.device.index or 0, seed=seed, lib_path=lib)
        N = self.n_envs
        z = self._zeros
        self.qpos, self.qvel, self.ctrl, self.warm = z(20, N), z(18, N), z(6, N), z(18, N)
        self.ring, self.ep_return = z(native.RING_DEPTH, 6, N), z(N)
        self.step_count, self.episode = z(N, dt=torch.int32), z(N, dt=torch.int32)
        self.obs, self.reward, self.discount = z(N, native.OBS_DIM), z(N), z(N)
        self.step_type = z(N, dt=torch.uint8)
        self._pack = None
        if N == 1:
            # ONE env (the reference's own use: run_eval.py, the notebooks): state and per-step outputs are views of one 256-byte buffer, so that a
            # step hands everything the numpy observation needs back to the host in ONE copy into pinned memory (round 4: six device-to-host
            # round trips per step, 0.45 ms of the 2.2 ms)
            self._pack = z(64)
            self.qpos, self.qvel = self._pack[0:20].view(20, 1), self._pack[20:38].view(18, 1)
            self.obs, self.reward, self.discount = self._pack[38:56].view(1, 18), self._pack[56:57], self._pack[57:58]
            self.step_type = self._pack[58:59].view(torch.uint8)[0:1]
            self._host = torch.zeros(64, dtype=torch.float32).pin_memory()
            self._act_host = torch.zeros(1, native.ACT_DIM, dtype=torch.float32).pin_memory()
        self._action = z(N, native.ACT_DIM)
        # per-env mass / inertia scale of (object, container): domain randomisation, 1.0 = the model's props
        self.mass_scale = torch.ones(2, N, dtype=torch.float32, device=self.device)
        self._events = torch.zeros(native.NEVENTS, dtype=torch.int64, device=self.device)
        self._pool = None
        self.sim.bind(*(t.data_ptr() for t in (self.qpos, self.qvel, self.ctrl, self.warm, self.ring,
                                                 self.ep_return, self.step_count, self.episode, self.mass_scale)))
        # physics_state / delayed_physics_state (so100_task.py:203-210,366-368; the reference enables them together with the
        # cameras): device-side 15-step delay line, on request - the throughput configurations are proprioceptive only
        if physics_state:
            self._bind_physics_state(native.PS_DELAY, native.PS_DIM)
        nsub = int(round(task.control_timestep / PHYSICS_TIMESTEP))
        last = scenes.time_limit_last_step(time_limit, task.control_timestep, PHYSICS_TIMESTEP) if np.isfinite(time_limit) else 1 << 30
        self.last_step = last
        self.sim.configure(action_offset=[float(x) for x in task.calibration.homing_offsets], last_step=last,
                           n_substeps=nsub, solver_iterations=int(solver_iterations),
                           solver_tolerance=float(solver_tolerance), settle_max_substeps=int(settle_max_substeps),
                           terminate_on_success=int(task.terminate_episode), env_id_base=int(env_id_base),
                           solver={"newton": native.SOLVER_NEWTON, "pgs": native.SOLVER_PGS}[str(solver).lower()],
                           prefetch_resets=int(bool(prefetch_resets)))
        self.physics = _PhysicsView(self)
        self._physics = self.physics
        self._store = None
        # what a settled reset state depends on besides (env id, episode) and the mass scale: the key of the on-disk store
        self._settle_key = dict(
            blob_sha256=hashlib.sha256(blob).hexdigest(), seed=seed, env_id_base=int(env_id_base), n_envs=N,
            solver=str(solver).lower(), narrowphase=narrowphase, solver_iterations=int(solver_iterations), solver_tolerance=float(solver_tolerance),
            settle_max_substeps=int(settle_max_substeps), action_offset=[float(x) for x in task.calibration.homing_offsets])

    # ------------------------------------------------------------------ specs
    def action_spec(self) -> BoundedArray:
        return so100_action_spec(self.task.rotation_joint_limit)

    def observation_spec(self):
        spec = collections.OrderedDict()
        spec["commanded_joints_pos"] = Array((6,), np.float64, "commanded_joints_pos")
        spec["joints_pos"] = Array((6,), np.float64, "joints_pos")
        spec["joints_vel"] = Array((0,), np.float64, "joints_vel")
        with_state = self.physics_state is not None or (self.n_envs == 1 and self.task.image_observation_enabled)
        if with_state:
            spec["physics_state"] = Array((38,), np.float64, "physics_state")
        spec["undelayed_joints_pos"] = Array((6,), np.float64, "undelayed_joints_pos")
        spec["undelayed_joints_vel"] = Array((0,), np.float64, "undelayed_joints_vel")
        if with_state:
            spec["delayed_physics_state"] = Array((38,), np.float64, "delayed_physics_state")
        return spec

    def _load_blob(self, real: str):
        return scenes.load_blob(self.task.object_name, real)

    def _debug_layout(self):
        return native.DBG, native.DEBUG_DIM

    # ------------------------------------------------------------------ stepping (tensors in, tensors out)
    def reset_all(self):
        self.sim.reset(None, self._stream())
        N = self.n_envs
        self.obs[:, 0:6] = self.qpos[0:6].t()
        self.obs[:, 6:12] = self.qpos[0:6].t()
        self.obs[:, 12:18] = self.ctrl.t()
        self.step_type.zero_()
        self.reward.zero_()
        self.discount.fill_(1.0)
        return self.obs

    def step_tensor(self, action):
        """action: float tensor [N, 6] on the device. Fills and returns (obs, reward, discount, step_type)."""
        torch = self.torch
        if action.shape != (self.n_envs, 6):
            raise ValueError(f"Expected 6 joint positions, got {tuple(action.shape)}")
        self._action.copy_(action)
        self.sim.step(self._action.data_ptr(), self.obs.data_ptr(), self.reward.data_ptr(), self.discount.data_ptr(),
                      self.step_type.data_ptr(), self._stream())
        return self.obs, self.reward, self.discount, self.step_type

    def _obs_dict(self):
        o = collections.OrderedDict()
        o["commanded_joints_pos"] = self.obs[:, 12:18]
        o["joints_pos"] = self.obs[:, 0:6]
        o["joints_vel"] = self.obs[:, 0:0]
        if self.physics_state is not None:
            o["physics_state"] = self.physics_state
        o["undelayed_joints_pos"] = self.obs[:, 6:12]
        o["undelayed_joints_vel"] = self.obs[:, 0:0]
        if self.physics_state is not None:
            o["delayed_physics_state"] = self.delayed_physics_state
        return o

    def reset(self) -> TimeStep:
        self.reset_all()
        return TimeStep(self.step_type, None, None, self._obs_dict())

    def step(self, action) -> TimeStep:
        torch = self.torch
        a = torch.as_tensor(action, dtype=torch.float32, device=self.device)
        if a.dim() == 1:
            a = a.unsqueeze(0)
        self.step_tensor(a)
        return TimeStep(self.step_type, self.reward, self.discount, self._obs_dict())

    def begin_episode(self):
        """Start an episode from the state currently in `qpos` / `qvel` (no placement, no settle)."""
        self.sim.begin_episode(self._stream())
        self.obs[:, 0:6] = self.qpos[0:6].t()
        self.obs[:, 6:12] = self.qpos[0:6].t()
        self.obs[:, 12:18] = self.ctrl.t()
        self.step_type.zero_()

    def set_mass_scale(self, scale):
        """scale: [2, N] (object, container) multipliers of the props' mass and inertia.  Flushes the reset prefetch
        (cached initial states were settled with the old masses)."""
        scale = self.torch.as_tensor(scale, dtype=self.torch.float32, device=self.device).reshape(2, self.n_envs)
        if not bool((scale > 0).all()):
            raise ValueError("mass scales must be positive")
        self.mass_scale.copy_(scale)
        if self._store is not None:
            self.set_settled_store(None)       # a settled-state store belongs to the old masses as well
        self.sim.configure()

    def set_reset_pool(self, qpos=None, qvel=None, ctrl=None):
        """Resets draw the initial state from this pool ([20, K], [18, K], [6, K] device tensors) instead of the
        reference's placement + settle; None restores the reference behaviour."""
        if qpos is None:
            self._pool = None
            self.sim.set_reset_pool(None, None, None, 0)
            return
        t = self.torch
        pool = tuple(t.as_tensor(a, dtype=t.float32, device=self.device).contiguous() for a in (qpos, qvel, ctrl))
        K = pool[0].shape[1]
        assert pool[0].shape == (20, K) and pool[1].shape == (18, K) and pool[2].shape == (6, K)
        self._pool = pool                      # keeps the tensors alive while the library reads them
        self.sim.set_reset_pool(pool[0].data_ptr(), pool[1].data_ptr(), pool[2].data_ptr(), K)

    # ------------------------------------------------------------------ settled-state store
    def settled_cache_key(self) -> dict:
        from . import build
        key = dict(self._settle_key)
        key["mass_scale_sha256"] = hashlib.sha256(self.mass_scale.detach().cpu().numpy().tobytes()).hexdigest()
        key["build"] = build.source_hash(mpr=self.narrowphase == "mpr")       # settled states are only bit-identical within one build of the kernels
        return key

    def compute_settled(self, n_episodes: int, first_episode: int = 0):
        """Placement + settle of episodes first_episode .. first_episode + n_episodes - 1 of every env, without touching
        the envs.  Returns device tensors (qpos [E,20,N], qvel [E,18,N], warmstart [E,18,N], flags [E,N])."""
        t, N, E = self.torch, self.n_envs, int(n_episodes)
        out = (t.zeros(E, 20, N, device=self.device), t.zeros(E, 18, N, device=self.device), t.zeros(E, 18, N, device=self.device),
               t.zeros(E, N, dtype=t.int32, device=self.device))
        self.sim.compute_settled(first_episode, E, *(a.data_ptr() for a in out), self._stream())
        return out

    def set_settled_store(self, tables=None, first_episode: int = 0):
        """Resets of the covered episodes copy their entry instead of settling (bit-identical); None detaches."""
        if tables is None:
            self._store = None
            self.sim.set_settled_store(None, None, None, None, 0, 0)
            return
        t, N = self.torch, self.n_envs
        q, v, w, f = tables
        q, v, w = (t.as_tensor(a, dtype=t.float32, device=self.device).contiguous() for a in (q, v, w))
        f = t.as_tensor(f, dtype=t.int32, device=self.device).contiguous()
        E = f.shape[0]
        assert q.shape == (E, 20, N) and v.shape == (E, 18, N) and w.shape == (E, 18, N) and f.shape == (E, N)
        self._store = (q, v, w, f)             # keeps the tensors alive while the library reads them
        self.sim.set_settled_store(q.data_ptr(), v.data_ptr(), w.data_ptr(), f.data_ptr(), int(first_episode), E)

    def save_settled_cache(self, path: str, n_episodes: int, first_episode: int = 0):
        """Computes the settled states of n_episodes episodes per env, writes them to `path` and attaches them."""
        from . import settled_cache
        tables = self.compute_settled(n_episodes, first_episode)
        names = [a[0] for a in settled_cache.ARRAYS]
        settled_cache.write(path, self.settled_cache_key(), first_episode, {n: a.cpu().numpy() for n, a in zip(names, tables)})
        self.set_settled_store(tables, first_episode)

    def load_settled_cache(self, path: str):
        """Attaches a file written by save_settled_cache(); refuses one computed for a different model, seed, shard,
        mass scale, solver setting or build (settled_cache.SettledCacheError names the differing fields)."""
        from . import settled_cache
        header, arrays = settled_cache.read(path, expect_key=self.settled_cache_key())
        self.set_settled_store(tuple(arrays[a[0]] for a in settled_cache.ARRAYS), header["first_episode"])
        return header

    # ------------------------------------------------------------------ depth / segmentation cameras (cameras.py)
    def render_depth(self, camera, height: int, width: int, env_ids=None, segmentation: bool = True):
        """Depth and geom-id images of the collision geometry at the current state, by ray casting on the GPU (so101_render).

        camera: a name of cameras.SO100_CAMERAS, a cameras.Camera, or a sequence of either (at most 8).
        env_ids: env indices to render (sequence or tensor), None = all.
        Returns (depth [n, ncam, height, width] float32, seg int32 of the same shape or None) on the env's device.  depth is the
        distance along the optical axis, +inf where the ray hits nothing; seg the geom index (`meta["geom_names"][i]` names it),
        -1 where it hits nothing.  This is not RGB: textures and visual-only meshes are not rendered."""
        from . import cameras as _cameras
        return self._render_depth(_cameras.resolve(camera), height, width, env_ids, segmentation)

    # ------------------------------------------------------------------ colour cameras (appearance.py: ColorCameras)
    _scene_shading = _appearance.SO100_SHADING

    def _scene_colors(self):
        return _appearance.so100_colors(self.meta)

    def render_color(self, camera, height: int, width: int, env_ids=None, colors=None, shading=None, normals: bool = False, depth: bool = False,
                     segmentation: bool = False):
        """Colour images of the collision geometry at the current state, by ray casting and shading on the GPU (so101_render_color).

        camera, env_ids: as in render_depth.  colors: None (the scene's table, appearance.so100_colors), a float32 [ngeom, 3] array or
        tensor, [n_envs, ngeom, 3] for colours per env (the rendered env's row is used), or a dict {anything geom_group() takes: rgb}
        applied over the scene's table.  shading: an appearance.Shading, None = appearance.SO100_SHADING.
        Returns appearance.ColorImages(rgb, normal, depth, seg) on the env's device: rgb uint8 [n, ncam, height, width, 3]; with
        normals=True the world-frame unit surface normal float32 [n, ncam, height, width, 3] (0 where the ray hits nothing); with
        depth / segmentation what render_depth returns, bit for bit; None otherwise.  This is not MuJoCo's renderer: what is drawn is
        the collision geometry of render_depth, flat-coloured per geom and Lambert-shaded by directional lights - no textures, shadows,
        specular term, visual-only meshes or positional lights."""
        from . import cameras as _cameras
        return self._render_color(_cameras.resolve(camera), height, width, env_ids, colors, shading, normals, depth, segmentation)

    # ------------------------------------------------------------------ Cartesian tool control (tools.py)
    def _resolve_tool(self, tool):
        from . import tools as _tools
        if getattr(self, "_tools", None) is None:
            self._tools = _tools.so100_tools(self.meta, self._model())
        return _tools.resolve(tool, self._tools)

    def _tool_columns(self, t):
        return 6

    def _ik_config(self, t, mode, config):
        return self.sim.ik_config(mode=mode, **config)

    def tool_pose(self, tool="fixed_jaw_pad", env_ids=None, q=None, jacobian: bool = False):
        """World pose of a tool frame (tools.Tool or a name of the scene's tools) on the GPU (so101_tool_pose): at the current qpos of
        the envs `env_ids` (None = all), or at explicit joint angles `q` [n, 6].  Returns (pos [n, 3], mat [n, 3, 3]) and, with
        jacobian=True, jac [n, 6, 6] - rows 0-2 the translational, rows 3-5 the rotational Jacobian of MuJoCo's mj_jacSite."""
        return self._tool_pose(tool, env_ids, q, jacobian)

    def solve_ik(self, target_pos, target_mat=None, tool="fixed_jaw_pad", mode=None, q_init=None, env_ids=None, **config):
        """Joint angles that bring a tool to Cartesian targets, one damped least-squares solve per row on the GPU (so101_tool_ik).

        target_pos [n, 3]; target_mat [n, 3, 3] or None.  mode: 0 position only, 1 position and the direction of the tool's z axis,
        2 position and full orientation; None = 0 without target_mat, else 1.  q_init [n, 6] starts the solves; None starts them
        from the current qpos of the envs `env_ids` (None = envs 0 .. n - 1).  **config replaces fields of the default settings
        (max_iters, tol_pos, tol_rot, rot_weight, damping, max_step, q_lo, q_hi; include/so101.h so101_ik_config).
        Returns (q [n, 6], converged [n] bool, residual [n, 2] = position error in metres and orientation error in radians at q,
        iters [n] int32, -1 where not converged).  Joints beyond the tool's link keep their starting value."""
        return self._solve_ik(target_pos, target_mat, tool, mode, q_init, env_ids, config)

    def cartesian_action(self, target_pos, target_mat=None, jaw=None, tool="fixed_jaw_pad", mode=None, **config):
        """An [N, 6] action for step_tensor() that commands the tool of every env to a Cartesian target: the IK solution started
        from the current qpos (solve_ik), with column 5 replaced by `jaw` (scalar or [N]) when given, minus the configured
        action_offset - the step computes ctrl = action + offset in float32, so the commanded ctrl is the solution: bit for bit
        with zero offsets and wherever float32 has an action whose sum with the offset rounds to the solution (the rounded
        difference is that action: 98.6 % of random joint angles with offsets of a few hundredths), else one unit in the last
        place beside it.  Targets the solve does not reach still give its last iterate: check solve_ik() where that matters."""
        torch = self.torch
        q, _, _, _ = self.solve_ik(target_pos, target_mat, tool=tool, mode=mode, **config)
        if q.shape[0] != self.n_envs:
            raise ValueError(f"cartesian_action needs one target per env ({self.n_envs}), got {q.shape[0]}")
        if jaw is not None:
            q[:, 5] = self._f32(jaw)
        offset = torch.tensor([float(x) for x in self.sim.cfg.action_offset], dtype=torch.float32, device=self.device)
        return q - offset

    # ------------------------------------------------------------------ contact sensing (contacts.py: ContactSensing)
    _geom_limit = _contacts.MAX_GEOMS
    _contact_capacity = native.MAXCON

    def _geom_groups(self):
        if getattr(self, "_groups", None) is None:
            self._groups = _contacts.so100_groups(self.meta, self._model())
        return self._groups

    def geom_group(self, spec):
        """A contacts.GeomGroup from a group name of the scene ("gripper", "arm", "props", "fixed_jaw_pads", "moving_jaw_pads", every body name),
        a geom name, an fnmatch pattern over the geom names, an iterable of geom ids or a GeomGroup."""
        return self._geom_group(spec)

    def contacts(self, env_ids=None, forces: bool = False):
        """The contact lists of the envs `env_ids` (None = all) at their current state, on the GPU (so101_contacts): a
        contacts.ContactReport of tensors on the env's device - count [n], flags [n] (1 candidate overflow, 2 contact overflow, 128 reduced
        to one contact per geom pair: the 64-contact capacity rule), geom [n, 64, 2], dist [n, 64], pos [n, 64, 3], frame [n, 64, 3, 3] (rows:
        normal geom1 -> geom2 and two tangents, MuJoCo's contact.frame) and, with forces=True, force [n, 64, 6] (mj_contactForce), else None.
        Slots beyond count hold geoms -1, dist +inf, zeros.  The forces are those of a forward pass at the current state (constraint rows and
        solve, warmstart read and left alone), not the impulses of the last substep; without forces only kinematics and collision run."""
        return self._contacts(env_ids, forces)

    def touch(self, pairs, env_ids=None, forces: bool = False):
        """Who touches whom: `pairs` is a sequence of at most 16 (a, b), each side anything geom_group() takes.  Per env of `env_ids` (None = all)
        and pair, reduced on the GPU from the env's contact list: a contacts.TouchReport of count [n, npair] int32 (contacts with one geom in a
        and the other in b), touching = count > 0, dist [n, npair] (the smallest, +inf without a contact) and, with forces=True,
        normal_force [n, npair] (sum of the normal forces) and force [n, npair, 3] (the net world-frame force ON group a), else None."""
        return self._touch(pairs, env_ids, forces)

    # ------------------------------------------------------------------ proximity sensing (proximity.py: ProximitySensing)
    def proximity(self, pairs, env_ids=None, q=None, max_dist: float = 0.1):
        """How far apart: `pairs` is a sequence of 1 to 16 (a, b), each side anything geom_group() takes.  Per entry and pair, on the GPU
        (so101_proximity), a proximity.ProximityReport of tensors on the env's device: dist [n, P], geom [n, P, 2] int32, point [n, P, 2, 3],
        normal [n, P, 3], flags [n, P] int32.

        Entries: the envs `env_ids` (None = all; an env may repeat).  With `q` [n, 6] - arm joint angles, the qpos[0:6] convention of
        tool_pose(q=...) - entry i is evaluated with the props of env env_ids[i] where they are now and the arm at q[i]; env_ids = [e] * K
        checks a K-waypoint trajectory against one env in one call.  Nothing bound is modified: qpos, qvel, ctrl and the warmstart stay.

        Per entry and pair, over every geom pair (one geom in a, the other in b) the model's own pair list admits - the list the collision
        stage walks, without same-body and excluded pairs, so "proximity < 0" and "touch" speak about the same pairs: `dist` is the smallest
        signed distance.  Separated: the Euclidean gap of the two surfaces, >= 0.  Penetrating: the smallest contact dist of the narrowphase for
        that geom pair (< 0, the number touch() gives), flags bit 1.  `geom`: the winning pair, the a-side geom first.  `point`: the closest
        point on the a-side geom and on the b-side geom, world frame (penetrating: the contact position offset by -+ dist / 2 along the
        normal).  `normal`: unit vector from the a point to the b point (penetrating: the contact normal, oriented from a to b).  Nothing
        below `max_dist` (a finite number above 0, at most 10 m), or no admitted pair: dist = max_dist, geom -1, zeros, flags bit 4 - what
        mj_geomDistance does with distmax.  flags bit 2: the distance iteration hit its cap on the winning pair, dist is an upper bound.
        Ties go to the pair that comes first in the model's pair list."""
        return self._proximity(pairs, env_ids, q, max_dist)

    def events(self, clear: bool = False) -> dict:
        """Counts since creation (or the last clear) of env-steps / env-resets that raised a flag: contact or candidate
        overflow, physics divergence (episode ended like a dm_control PhysicsError), rejected placement, unsettled
        reset.  See so101_get_events in include/so101.h."""
        self.sim.get_events(self._events.data_ptr(), clear, self._stream())
        v = self._events.cpu().tolist()
        return dict(zip(native.EVENT_NAMES, v))

    def episode_returns(self):
        out = self.torch.empty_like(self.ep_return)
        self.sim.get_returns(out.data_ptr(), self._stream())
        return out

    def diagnostics(self):
        d = self.torch.zeros(self.n_envs, native.DIAG_DIM, dtype=self.torch.int32, device=self.device)
        self.sim.get_diag(d.data_ptr(), self._stream())
        return d


class SingleEnvironment(BatchedEnvironment):
    """N = 1 facade with the reference's numpy observation dict (keys/order:
    examples/so101_rl_breakdown.ipynb:65; shapes :115-122).

    Seed compatibility: the reference's placements come from `np.random.RandomState(seed)` inside dm_control's
    PropPlacer.  With `seed_compatible=True` (default) this facade draws them from the same generator in the same
    order - object position `uniform(low, high)` (3 draws, so100_hand_over.py:37-41), object yaw (1, :42-49),
    container position (3 per attempt, at most 20 attempts against collisions, :51-55 / :216-221) - writes them into
    the state and lets the kernels settle (so101_settle) and start the episode.  An int seed or a RandomState therefore
    reproduces the reference's initial placements; the batched environments key a counter RNG by (seed, env id,
    episode) instead."""

    def __init__(self, task, seed_compatible: bool = True, random_state=None, **kw):
        self._seed_compatible = bool(seed_compatible)
        self._np_random = generator_of(random_state)
        if self._seed_compatible:
            kw.setdefault("prefetch_resets", False)      # the host draws the placements: nothing the kernels could settle ahead of time
        kw.pop("physics_state", None)                    # N = 1 keeps the reference's rule (image_observation_enabled) and a host-side line
        super().__init__(task, n_envs=1, random_state=(random_state if not isinstance(random_state, np.random.RandomState) else 0), **kw)
        self._state_ring = collections.deque(maxlen=_PHYSICS_DELAY_STEPS)
        self._pending_first = False
        self._placer = self._hand_over_placer()
        # a stream of its own: the library replays the step's launch chain as a captured HIP graph on any stream but the legacy null stream
        self._own = self.torch.cuda.Stream(device=self.device)

    def _join_caller(self):
        """Order the env's own stream behind the caller's current stream: the constructor's fills, `bind` / `configure`, and every
        inherited mutator (`set_mass_scale`, `set_reset_pool`, `begin_episode`, `step_tensor`, `compute_settled`) are enqueued on the stream
        that is current when they are called, and torch creates `_own` non-blocking - without this edge `env.set_mass_scale(t); env.reset()`
        would race on qpos / mass_scale / the record.  The other direction needs no event: `_fetch()` synchronises `_own` on the host
        before reset() / step() return, so whatever the caller enqueues afterwards starts after this env's work."""
        cur = self.torch.cuda.current_stream(self.device)
        if cur != self._own:
            self._own.wait_stream(cur)

    def _fetch(self):
        """the 256-byte state + output record of the last call -> pinned host memory, one copy, one synchronisation; returns the numpy view"""
        self._host.copy_(self._pack, non_blocking=True)
        self.torch.cuda.current_stream(self.device).synchronize()
        return self._host.numpy()

    # ---- reference-order placement + settle
    def _reset_seed_compatible(self):
        torch = self.torch
        self._place_hand_over(np.zeros(20), 6, 13)
        before = self.events()["settle_not_converged"]          # (cumulative counters stay what events() documents)
        # settle with the controls the episode starts with (ctrl = home + offsets), like the kernels' own reset
        home = np.asarray(scenes.SO100_HOME_CTRL, dtype=np.float64)
        self.ctrl.copy_(torch.as_tensor(home + np.asarray(self.task.calibration.homing_offsets, dtype=np.float64),
                                        dtype=torch.float32, device=self.device).unsqueeze(1))
        self.sim.settle(self._stream())
        self.begin_episode()
        if self.events()["settle_not_converged"] > before:
            import warnings
            warnings.warn(SETTLE_WARNING)

    def _np_obs(self, first: bool, h=None):
        h = self._fetch() if h is None else h
        ob = h[38:56].astype(np.float64)
        o = collections.OrderedDict()
        o["commanded_joints_pos"] = ob[12:18].copy()
        o["joints_pos"] = ob[0:6].copy()
        o["joints_vel"] = np.zeros((0,), dtype=np.float64)
        if self.task.image_observation_enabled:
            state = h[0:38].astype(np.float64)
            if first:
                self._state_ring.clear()
                self._state_ring.extend([state] * _PHYSICS_DELAY_STEPS)   # INITIAL_VALUE padding
            delayed = self._state_ring[0]
            self._state_ring.append(state)
            o["physics_state"] = state
        o["undelayed_joints_pos"] = ob[6:12].copy()
        o["undelayed_joints_vel"] = np.zeros((0,), dtype=np.float64)
        if self.task.image_observation_enabled:
            o["delayed_physics_state"] = delayed
        return o

    def reset(self) -> TimeStep:
        self._join_caller()
        with self.torch.cuda.stream(self._own):
            if self._seed_compatible and self._pool is None:
                self._reset_seed_compatible()
            else:
                self.reset_all()
            self._pending_first = False
            return TimeStep(StepType.FIRST, None, None, self._np_obs(first=True))

    def step(self, action) -> TimeStep:
        a = np.asarray(action, dtype=np.float64).reshape(-1)
        if len(a) != 6:
            raise ValueError(f"Expected 6 joint positions, got {len(a)}")
        if self._pending_first:            # the step after LAST restarts the episode and reports FIRST (dm_control)
            return self.reset()
        self._join_caller()
        with self.torch.cuda.stream(self._own):
            self._act_host[0] = self.torch.from_numpy(a)
            self._action.copy_(self._act_host, non_blocking=True)
            self.sim.step(self._action.data_ptr(), self.obs.data_ptr(), self.reward.data_ptr(), self.discount.data_ptr(),
                          self.step_type.data_ptr(), self._stream())
            h = self._fetch()
        st = StepType(int(h[58:59].view(np.uint8)[0]))
        if st == StepType.LAST and self._seed_compatible and self._pool is None:
            self._pending_first = True     # the host draws the next placements; the kernels' own auto-reset is not used
        if st == StepType.FIRST:
            return TimeStep(st, None, None, self._np_obs(first=True, h=h))
        return TimeStep(st, float(h[56]), float(h[57]), self._np_obs(first=False, h=h))
