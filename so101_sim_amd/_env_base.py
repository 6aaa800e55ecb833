"""What the environments of env.py (SO100 engine) and aloha.py (general-tree engine) share around their step paths: device, seed and library
resolution, the unpacked model, hull planes and the depth render, the seed-compatible hand-over placement, the physics-state line, and the
keywords the task classes have in common.  The step paths themselves stay in the two modules."""
from __future__ import annotations

import os

import numpy as np

from . import appearance as _appearance
from . import contacts as _contacts
from . import proximity as _proximity
from .tool_control import ToolControl

DEFAULT_CONTROL_TIMESTEP = 0.02
PHYSICS_TIMESTEP = 0.002
SETTLE_WARNING = "Failed to settle physics within the settle budget (dm_control warns likewise)"


def pop_task_keywords(task, kwargs):
    """The keywords every task class takes, with the reference's defaults"""
    task.control_timestep = float(kwargs.pop("control_timestep", DEFAULT_CONTROL_TIMESTEP))
    task.cameras = tuple(kwargs.pop("cameras", ()))
    task.image_observation_enabled = bool(kwargs.pop("image_observation_enabled", True))
    task.terminate_episode = bool(kwargs.pop("terminate_episode", True))


def generator_of(random_state) -> np.random.RandomState:
    """numpy's generator of a seed-compatible single env: the caller's RandomState itself, else one seeded with the int (None: from the OS)"""
    if isinstance(random_state, np.random.RandomState):
        return random_state
    return np.random.RandomState() if random_state is None else np.random.RandomState(int(random_state))


class EnvironmentBase(ToolControl, _contacts.ContactSensing, _proximity.ProximitySensing, _appearance.ColorCameras):
    """Subclasses supply `_load_blob(real)` -> (blob bytes, meta) and `_debug_layout()` -> (layout of the handle's debug_forward row, its width)."""

    def _open_device(self, task, n_envs, device, random_state, host_draws: bool = False):
        """torch, task, n_envs, device and seed.  host_draws: a single env that draws its placements from the caller's RandomState leaves the
        generator untouched and hands the kernels seed 0"""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("so101_sim_amd needs a ROCm GPU (MI355X): the step path has no CPU fallback")
        self.torch = torch
        self.task = task
        self.n_envs = int(n_envs)
        self.device = torch.device(device if device is not None else "cuda:0")
        if isinstance(random_state, np.random.RandomState):
            seed = 0 if host_draws else int(random_state.randint(0, 2**31 - 1))
        elif random_state is None:
            seed = int.from_bytes(os.urandom(4), "little")
        else:
            seed = int(random_state)
        self.seed = seed
        self._models = {}
        self._dbg = None
        self.physics_state = self.delayed_physics_state = self._ps_ring = None

    def _zeros(self, *shape, dt=None):
        return self.torch.zeros(*shape, dtype=dt or self.torch.float32, device=self.device)

    def _model(self, real: str = "f32") -> dict:
        """The unpacked model blob, "f32" (what the kernels hold) or "f64" (the placers' bounds unrounded), unpacked once"""
        if real not in self._models:
            from .model import blob as blobfmt
            self._models[real] = blobfmt.unpack(self._load_blob(real)[0])
        return self._models[real]

    def _narrowphase_library(self, narrowphase: str, env_names_library: bool = False):
        """Checks and records `narrowphase`; returns the library path for the handle, None = native.LIB_PATH.  "epa" (default): the penetration
        of non-flat convex pairs is the minimum translation (MPR's final portal expanded by EPA to the nearest face of the Minkowski difference,
        as mujoco >= 3.3's native GJK / EPA reports it - the reference pins mujoco>=3.3.3, requirements.txt:7).  "mpr": the -DSO101_MPR build of
        the library (built on demand) keeps MPR's portal depth: 5-15 % faster, 3x the physics errors under random actions (DESIGN.md section 4,
        profiles/README.md).  env_names_library: SO101_HIP_LIB - kernel experiments, bench.py --pipeline 2|3 - names the library whatever the
        narrowphase: whoever sets it built the variant it wants, e.g. build(exp=True, mpr=True)."""
        if narrowphase not in ("mpr", "epa"):
            raise ValueError(f"narrowphase must be 'mpr' or 'epa', got {narrowphase!r}")
        self.narrowphase = narrowphase
        if narrowphase != "mpr" or (env_names_library and os.environ.get("SO101_HIP_LIB")):
            return None
        from . import build as _build
        return _build.build(mpr=True)

    def _bind_physics_state(self, depth: int, dim: int):
        """physics_state / delayed_physics_state [N, dim] and their device-side delay line of `depth` control steps"""
        self._ps_ring = self._zeros(depth, dim, self.n_envs)
        self.physics_state, self.delayed_physics_state = self._zeros(self.n_envs, dim), self._zeros(self.n_envs, dim)
        self.sim.bind_physics_state(self._ps_ring.data_ptr(), self.physics_state.data_ptr(), self.delayed_physics_state.data_ptr())

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def synchronize(self):
        """Wait until everything this env was asked to do on the caller's current stream is done (steps, resets, reads).  Cheaper than
        `torch.cuda.synchronize()` right after a mass reset: a device-wide synchronise also waits for the library's background reset
        prefetch - settled initial states of FUTURE episodes, up to ~2 s of low-priority work on 256 wavefronts for 4096 envs - which no
        result of the calls made so far depends on (bench.py reports both clocks, `sustained.host_env_steps_per_s` / `env_steps_per_s`)."""
        self.torch.cuda.current_stream(self.device).synchronize()

    def close(self):
        self.sim.close()

    # ------------------------------------------------------------------ depth / segmentation cameras (cameras.py)
    def _ensure_hull_planes(self):
        """Facet planes of the mesh geoms' hulls, computed from the blob's vertices and handed to the library on first use"""
        if getattr(self, "_planes_set", False):
            return
        from .model import meshes
        m = self._model()
        verts = np.asarray(m["mesh_vert"], dtype=np.float64).reshape(-1, 3)
        adr, chunks = [0], []
        for t, a, n in zip(m["geom_type"], m["geom_vertadr"], m["geom_vertnum"]):
            if int(t) == 5:
                chunks.append(meshes.hull_planes(verts[a:a + n]))
            adr.append(adr[-1] + (len(chunks[-1]) if int(t) == 5 else 0))
        planes = np.concatenate(chunks) if chunks else np.zeros((0, 4))
        with self.torch.cuda.device(self.device):
            self.sim.set_hull_planes(planes.astype(np.float32), np.asarray(adr, dtype=np.int32))
        self._planes_set = True

    def _render_depth(self, cams, height, width, env_ids, segmentation, **source):
        """render_depth for resolved cameras; **source: the tree engine's `source`"""
        torch = self.torch
        self._ensure_hull_planes()
        idx, n = self._env_index(env_ids)
        depth = torch.empty(n, len(cams), int(height), int(width), dtype=torch.float32, device=self.device)
        seg = torch.empty(n, len(cams), int(height), int(width), dtype=torch.int32, device=self.device) if segmentation else None
        self.sim.render([c.spec() for c in cams], height, width, idx.data_ptr() if idx is not None else None, n,
                        depth.data_ptr(), seg.data_ptr() if seg is not None else None, self._stream(), **source)
        return depth, seg

    # ------------------------------------------------------------------ reference-order placement of a single env
    def _hand_over_placer(self) -> dict:
        """Bounds of the hand-over placement distributions (f64: the draws must be the reference's, bit for bit) and the container's geoms"""
        m, m64 = self._model(), self._model("f64")
        con_body = int(np.asarray(m["task_container_body"]).ravel()[0])
        f = lambda k: np.asarray(m64[k], dtype=np.float64)
        return dict(obj_lo=f("task_obj_pos_lo"), obj_hi=f("task_obj_pos_hi"), yaw=f("task_obj_yaw"), con_lo=f("task_con_pos_lo"),
                    con_hi=f("task_con_pos_hi"), con_geoms=set(np.nonzero(np.asarray(m["geom_body"]) == con_body)[0].tolist()))

    def _write_state(self, q):
        """q (host, [nq]) into the single env's qpos; qvel and the warmstart cleared"""
        torch = self.torch
        self.qpos.copy_(torch.as_tensor(q, dtype=torch.float32, device=self.device).unsqueeze(1))
        self.qvel.zero_()
        self.warm.zero_()

    def _container_collides(self) -> bool:
        """one forward pass at the bound state: does any contact involve a geom of the container?"""
        D, dim = self._debug_layout()
        if self._dbg is None:
            self._dbg = self._zeros(1, dim)
        self.sim.debug_forward(self._dbg.data_ptr(), self._stream())
        r = self._dbg[0].cpu().numpy()
        for k in range(int(r[D["COUNTS"]])):
            if int(r[D["CON"] + 10 * k + 7]) in self._placer["con_geoms"] or int(r[D["CON"] + 10 * k + 8]) in self._placer["con_geoms"]:
                return True
        return False

    def _place_hand_over(self, q, qo: int, qc: int):
        """dm_control's PropPlacers with numpy's generator, in the reference's order: object position `uniform(low, high)` (3 draws), object yaw
        (1), container position (3 per attempt, at most 20 attempts against collisions).  q: the qpos row with everything but the two props
        filled in; qo / qc: the qpos addresses of object and container.  Leaves the accepted state bound and `placements` set."""
        P, rs = self._placer, self._np_random
        opos = rs.uniform(P["obj_lo"], P["obj_hi"])                       # distributions.Uniform(low, high, single_sample=True)
        yaw = rs.uniform(P["yaw"][0], P["yaw"][1])                        # QuaternionFromAxisAngle(axis=z, angle=Uniform)
        q[qo:qo + 3] = opos
        q[qo + 3:qo + 7] = [np.cos(0.5 * yaw), 0.0, 0.0, np.sin(0.5 * yaw)]
        q[qc + 3] = 1.0
        for _ in range(20):                                               # PropPlacer max_attempts_per_prop
            q[qc:qc + 3] = rs.uniform(P["con_lo"], P["con_hi"])
            self._write_state(q)
            if not self._container_collides():
                break
        else:
            raise RuntimeError("Failed to place the container without collisions in 20 attempts (dm_control PropPlacer raises here too)")
        self.placements = dict(object_position=opos.copy(), object_yaw=float(yaw), container_position=q[qc:qc + 3].copy())
