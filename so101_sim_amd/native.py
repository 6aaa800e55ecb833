"""ctypes binding of libso101_hip.so (C ABI in include/so101.h).

The library is built in-tree by `__graft_entry__.build()` / `python -m so101_sim_amd.build`.  There is no
CPU fallback: if the shared object is missing or a call fails, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SO101_HIP_LIB") or os.path.join(_HERE, "csrc", "libso101_hip.so")      # (the variable: kernel experiments only)

SOLVER_PGS, SOLVER_NEWTON = 0, 1
OBS_DIM = 18
ACT_DIM = 6
RING_DEPTH = 5
DIAG_DIM = 8
PS_DIM, PS_DELAY = 38, 15
NEVENTS = 8
EVENT_NAMES = ("candidate_overflow", "contact_overflow", "arm_pool_overflow", "diverged", "placement_rejected",
               "settle_not_converged", "scheduler_abort", "contacts_reduced")
INFO = dict(graph_active=0, step_path=1, chains=2, hw_queues=3, scheduler_aborts=4, scratch_bytes=5, narrow_list_rows=6)
DEBUG_DIM = 2048
MAXCON = 64

# debug_forward layout (csrc/so101_kernels.hpp DBG_*)
DBG = dict(M=0, MINV=36, BIAS=72, SMOOTH=78, QACC=96, COUNTS=114, XPOS=120, CON=144, FORCE=144 + 10 * MAXCON,
           ROWF=144 + 16 * MAXCON, REWARD=144 + 16 * MAXCON + 16)


class Buffers(C.Structure):
    _fields_ = [("qpos", C.c_void_p), ("qvel", C.c_void_p), ("ctrl", C.c_void_p), ("warmstart", C.c_void_p),
                ("obs_ring", C.c_void_p), ("ep_return", C.c_void_p), ("step_count", C.c_void_p),
                ("episode", C.c_void_p), ("mass_scale", C.c_void_p)]


class Config(C.Structure):
    _fields_ = [("action_offset", C.c_float * ACT_DIM), ("last_step", C.c_int32), ("n_substeps", C.c_int32),
                ("solver_iterations", C.c_int32), ("solver_tolerance", C.c_float),
                ("settle_max_substeps", C.c_int32), ("terminate_on_success", C.c_int32),
                ("env_id_base", C.c_uint64), ("solver", C.c_int32), ("prefetch_resets", C.c_int32), ("pipeline", C.c_int32),
                ("groups", C.c_int32), ("use_graph", C.c_int32), ("chain_waves", C.c_int32)]


class CameraSpec(C.Structure):
    """so101_camera of include/so101.h"""
    _fields_ = [("body", C.c_int32), ("pos", C.c_float * 3), ("mat", C.c_float * 9), ("fovy_deg", C.c_float)]


def camera_array(cams):
    """(body, pos[3], mat[9] row-major, fovy_deg) tuples as the so101_camera array of so101_render / so101_tree_render"""
    arr = (CameraSpec * max(len(cams), 1))()
    for k, (body, pos, mat, fovy) in enumerate(cams):
        arr[k].body = int(body)
        arr[k].pos[:] = [float(x) for x in pos]
        arr[k].mat[:] = [float(x) for x in mat]
        arr[k].fovy_deg = float(fovy)
    return arr


MAX_LIGHTS = 4          # SO101_MAX_LIGHTS


class LightSpec(C.Structure):
    _fields_ = [("dir", C.c_float * 3), ("diffuse", C.c_float * 3), ("headlight", C.c_int32)]


class ShadingSpec(C.Structure):
    """so101_shading of include/so101.h"""
    _fields_ = [("ambient", C.c_float * 3), ("background", C.c_float * 3), ("nlight", C.c_int32), ("light", LightSpec * MAX_LIGHTS)]


class ColorOut(C.Structure):
    """so101_color_out of include/so101.h: device addresses, any may be None, not all"""
    _fields_ = [("rgb", C.c_void_p), ("normal", C.c_void_p), ("depth", C.c_void_p), ("seg", C.c_void_p)]


def shading_struct(shading) -> ShadingSpec:
    """(ambient[3], background[3], lights) -> so101_shading; a light is (dir[3] or None for a headlight, diffuse[3]).  A ShadingSpec passes through."""
    if isinstance(shading, ShadingSpec):
        return shading
    ambient, background, lights = shading
    lights = list(lights)
    if len(lights) > MAX_LIGHTS:
        raise ValueError(f"at most {MAX_LIGHTS} lights, got {len(lights)}")
    out = ShadingSpec()
    out.ambient[:] = [float(x) for x in ambient]
    out.background[:] = [float(x) for x in background]
    out.nlight = len(lights)
    for k, (direction, diffuse) in enumerate(lights):
        out.light[k].headlight = int(direction is None)
        out.light[k].dir[:] = [0.0, 0.0, 0.0] if direction is None else [float(x) for x in direction]
        out.light[k].diffuse[:] = [float(x) for x in diffuse]
    return out


class ToolSpec(C.Structure):
    """so101_tool of include/so101.h"""
    _fields_ = [("body", C.c_int32), ("pos", C.c_float * 3), ("mat", C.c_float * 9)]


class IkConfig(C.Structure):
    """so101_ik_config of include/so101.h"""
    _fields_ = [("mode", C.c_int32), ("max_iters", C.c_int32), ("tol_pos", C.c_float), ("tol_rot", C.c_float), ("rot_weight", C.c_float),
                ("damping", C.c_float), ("max_step", C.c_float), ("q_lo", C.c_float * 6), ("q_hi", C.c_float * 6)]


class TreeIkConfig(C.Structure):
    """so101_tree_ik_config of include/so101.h"""
    _fields_ = [("mode", C.c_int32), ("max_iters", C.c_int32), ("tol_pos", C.c_float), ("tol_rot", C.c_float), ("rot_weight", C.c_float),
                ("damping", C.c_float), ("max_step", C.c_float), ("free_mask", C.c_uint32), ("q_lo", C.c_float * 8), ("q_hi", C.c_float * 8)]


TOUCH_MAX_PAIRS = 16          # SO101_TOUCH_MAX_PAIRS
CONTACT_OUT_FIELDS = ("count", "flags", "geom", "dist", "pos", "frame", "force", "pair_count", "pair_dist", "pair_normal", "pair_force")


class GeomPair(C.Structure):
    """so101_geom_pair of include/so101.h: two 128-bit geom masks"""
    _fields_ = [("a", C.c_uint32 * 4), ("b", C.c_uint32 * 4)]


class ContactOut(C.Structure):
    """so101_contact_out of include/so101.h: raw device addresses, None = not wanted"""
    _fields_ = [(k, C.c_void_p) for k in CONTACT_OUT_FIELDS]


class TreeGeomPair(C.Structure):
    """so101_tree_geom_pair of include/so101.h: two 256-bit geom masks"""
    _fields_ = [("a", C.c_uint32 * 8), ("b", C.c_uint32 * 8)]


PROXIMITY_OUT_FIELDS = ("dist", "geom", "point", "normal", "flags", "queries")


class ProximityOut(C.Structure):
    """so101_proximity_out of include/so101.h: raw device addresses, None = not wanted"""
    _fields_ = [(k, C.c_void_p) for k in PROXIMITY_OUT_FIELDS]


def geom_pair_array(pairs, words: int = 4):
    """((a words, b words), ...) as the so101_geom_pair array of so101_contacts (words = 4) or the so101_tree_geom_pair array of
    so101_tree_contacts (words = 8)"""
    arr = ({4: GeomPair, 8: TreeGeomPair}[words] * max(len(pairs), 1))()
    for k, (a, b) in enumerate(pairs):
        arr[k].a[:] = [int(x) & 0xFFFFFFFF for x in a]
        arr[k].b[:] = [int(x) & 0xFFFFFFFF for x in b]
    return arr


TREE_TOOL_MAXCOL = 8          # columns of a tool's chain at most (so101_tree_tool_chain)
TREE_JNT_HINGE, TREE_JNT_SLIDE = 1, 3


def tool_spec(tool) -> ToolSpec:
    """(body, pos[3], mat[9] row-major) as a so101_tool"""
    body, pos, mat = tool
    t = ToolSpec()
    t.body = int(body)
    t.pos[:] = [float(x) for x in pos]
    t.mat[:] = [float(x) for x in mat]
    return t


class TreeConfig(C.Structure):
    _fields_ = [("n_substeps", C.c_int), ("last_step", C.c_int), ("settle_max_substeps", C.c_int), ("terminate_on_success", C.c_int),
                ("solver_iterations", C.c_int), ("solver_tolerance", C.c_float), ("seed", C.c_uint64), ("env_id_base", C.c_uint64),
                ("reward_mode", C.c_int), ("reward_requires_handover", C.c_int),
                ("joints_delay_steps", C.c_int), ("physics_delay_steps", C.c_int), ("prefetch_resets", C.c_int), ("pipeline", C.c_int)]


TREE_DBG = dict(COUNTS=0, BIAS=8, QSM=40, QACC=72, XPOS=104, M=200, CON=1224, FORCE=1864, MSTRIDE=32)     # the 32-dof build; TreeSim.dbg is the handle's own

# the struct(s) of include/so101.h each Structure mirrors (LightSpec: the unnamed element type of so101_shading.light)
C_STRUCTS = {Buffers: ("so101_buffers",), Config: ("so101_config",), CameraSpec: ("so101_camera",), ShadingSpec: ("so101_shading",),
             ColorOut: ("so101_color_out",), ToolSpec: ("so101_tool", "so101_tree_tool"), IkConfig: ("so101_ik_config",),
             TreeIkConfig: ("so101_tree_ik_config",), GeomPair: ("so101_geom_pair",), TreeGeomPair: ("so101_tree_geom_pair",),
             ContactOut: ("so101_contact_out",), ProximityOut: ("so101_proximity_out",), TreeConfig: ("so101_tree_config",)}


def _signatures():
    """export name -> (restype, argtypes): every prototype of include/so101.h, in its order (tests/test_abi_and_api.py compares the two)"""
    i, f, vp, P = C.c_int, C.c_float, C.c_void_p, C.POINTER
    cam, tool = P(CameraSpec), P(ToolSpec)
    sig = {
        "version": (i, []),
        "max_contacts": (i, []),
        "create": (i, [C.c_char_p, C.c_size_t, i, i, C.c_uint64, P(vp)]),
        "destroy": (None, [vp]),
        "default_config": (i, [P(Config)]),
        "configure": (i, [vp, P(Config)]),
        "bind_state": (i, [vp, P(Buffers)]),
        "bind_physics_state": (i, [vp, vp, vp, vp]),
        "reset": (i, [vp, vp, vp]),
        "set_reset_pool": (i, [vp, vp, vp, vp, i]),
        "compute_settled": (i, [vp, i, i, vp, vp, vp, vp, vp]),
        "set_settled_store": (i, [vp, vp, vp, vp, vp, i, i]),
        "settle": (i, [vp, vp]),
        "begin_episode": (i, [vp, vp]),
        "step": (i, [vp, vp, vp, vp, vp, vp, vp]),
        "physics": (i, [vp, i, i, vp]),
        "reward": (i, [vp, vp, vp]),
        "get_returns": (i, [vp, vp, vp]),
        "get_diag": (i, [vp, vp, vp]),
        "get_events": (i, [vp, vp, i, vp]),
        "debug_forward": (i, [vp, vp, vp]),
        "debug_stages": (i, [vp, vp, vp]),
        "debug_candidates": (i, [vp, vp, vp, vp, vp, vp]),
        "get_info": (C.c_longlong, [vp, i, vp]),
        "debug_chain_stats": (i, [vp, vp, i, vp]),
        "set_hull_planes": (i, [vp, vp, vp]),
        "render": (i, [vp, cam, i, i, i, vp, i, vp, vp, vp]),
        "render_color": (i, [vp, cam, i, i, i, vp, i, P(ShadingSpec), vp, i, P(ColorOut), vp]),
        "ik_default_config": (i, [vp, P(IkConfig)]),
        "tool_pose": (i, [vp, tool, vp, vp, i, vp, vp, vp, vp]),
        "tool_ik": (i, [vp, tool, P(IkConfig), vp, vp, vp, vp, i, vp, vp, vp, vp]),
        "contacts": (i, [vp, vp, i, i, P(GeomPair), i, P(ContactOut), vp]),
        "proximity": (i, [vp, vp, i, vp, P(GeomPair), i, f, P(ProximityOut), vp]),
        "last_error": (C.c_char_p, [vp]),
        "tree_create": (i, [C.c_char_p, C.c_size_t, i, i, P(vp)]),
        "tree_destroy": (None, [vp]),
        "tree_dims": (i, [vp, P(i)]),
        "tree_last_plan": (i, [vp, P(i)]),
        "tree_bind_state": (i, [vp, vp, vp, vp, vp]),
        "tree_configure": (i, [vp, i, f]),
        "tree_physics": (i, [vp, i, vp]),
        "tree_debug_forward": (i, [vp, vp, vp]),
        "tree_get_diag": (i, [vp, vp, vp]),
        "tree_obs_dim": (i, [vp]),
        "tree_bind_env": (i, [vp, vp, vp, vp, vp, vp]),
        "tree_configure_env": (i, [vp, P(TreeConfig)]),
        "tree_bind_physics_state": (i, [vp, vp, vp, vp]),
        "tree_reset": (i, [vp, vp, vp]),
        "tree_compute_settled": (i, [vp, i, i, vp, vp, vp, vp, vp]),
        "tree_set_settled_store": (i, [vp, i, i, vp, vp, vp, vp]),
        "tree_settle": (i, [vp, vp]),
        "tree_begin_episode": (i, [vp, vp]),
        "tree_step": (i, [vp, vp, vp, vp, vp, vp, vp]),
        "tree_set_hull_planes": (i, [vp, vp, vp]),
        "tree_render": (i, [vp, cam, i, i, i, vp, i, i, vp, vp, vp]),
        "tree_render_color": (i, [vp, cam, i, i, i, vp, i, i, P(ShadingSpec), vp, i, P(ColorOut), vp]),
        "tree_tool_chain": (i, [vp, i, vp, vp, vp]),
        "tree_ik_default_config": (i, [vp, i, P(TreeIkConfig)]),
        "tree_tool_pose": (i, [vp, tool, vp, vp, i, vp, vp, vp, vp]),
        "tree_tool_ik": (i, [vp, tool, P(TreeIkConfig), vp, vp, vp, vp, i, vp, vp, vp, vp]),
        "tree_contacts": (i, [vp, vp, i, i, P(TreeGeomPair), i, P(ContactOut), vp]),
        "tree_proximity": (i, [vp, vp, i, vp, P(C.c_int32), i, P(TreeGeomPair), i, f, P(ProximityOut), vp]),
        "tree_last_error": (C.c_char_p, [vp]),
    }
    return {"so101_" + k: v for k, v in sig.items()}


SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)

_libs: dict[str, C.CDLL] = {}


def load_library(path: str | None = None) -> C.CDLL:
    """The library at `path` (default LIB_PATH) with SIGNATURES applied, once per path: the product, its -DSO101_MPR / experimental builds and
    the emulated build alike"""
    path = path or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback for the step path.")
    # PyTorch bundles its own HIP runtime; it must be the first one the process loads, otherwise this
    # library binds /opt/rocm's copy and the two runtimes do not see each other's device state.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _libs[path] = L
    return L


class _Handle:
    """What Sim and TreeSim share: creation, close, the error check and the bodies of the calls the two engines have under both prefixes.
    The engine's foreign functions are resolved once per handle, as `_c_<name>` for `<_PREFIX><name>`; what differs between the engines
    beyond the prefix is a parameter (`_WORDS`, `source`, `q_adr`)."""
    _PREFIX = "so101_"
    _WORDS = 4            # 32-bit words of a geom mask: GeomPair / TreeGeomPair

    def _create(self, lib_path, blob_f32: bytes, n_envs: int, *args):
        self.L = load_library(lib_path)
        tree = self._PREFIX == "so101_tree_"
        for name in SIGNATURES:
            if name.startswith("so101_tree_") == tree:
                setattr(self, "_c_" + name[len(self._PREFIX):], getattr(self.L, name))
        self.n_envs = int(n_envs)
        h = C.c_void_p()
        rc = self._c_create(blob_f32, len(blob_f32), self.n_envs, *args, C.byref(h))
        if rc != 0:
            msg = self._c_last_error(None)
            raise RuntimeError(f"{self._PREFIX}create failed ({rc}): {msg.decode() if msg else '?'}")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self._c_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        """what: the entry point's name without the prefix"""
        if rc != 0:
            msg = self._c_last_error(self.h)
            raise RuntimeError(f"{self._PREFIX}{what} failed ({rc}): {msg.decode() if msg else '?'}")

    def bind_physics_state(self, ring, physics_state, delayed):
        self._check(self._c_bind_physics_state(self.h, *(C.c_void_p(x) if x else None for x in (ring, physics_state, delayed))), "bind_physics_state")

    def _set_hull_planes(self, planes, plane_adr):
        import numpy as np
        planes = np.ascontiguousarray(planes, dtype=np.float32).reshape(-1, 4)
        plane_adr = np.ascontiguousarray(plane_adr, dtype=np.int32)
        self._check(self._c_set_hull_planes(self.h, planes.ctypes.data, plane_adr.ctypes.data), "set_hull_planes")

    def _render(self, cams, height, width, env_index, n_render, depth, seg, stream, source=None):
        """source: None on the SO100 engine, whose call has no such argument"""
        self._check(self._c_render(self.h, camera_array(cams), len(cams), int(height), int(width), env_index, int(n_render),
                                   *(() if source is None else (int(source),)), depth, seg, stream), "render")

    def _render_color(self, cams, height, width, env_index, n_render, shading, geom_rgb, rgb_per_env, rgb, normal, depth, seg, stream, source=None):
        out = ColorOut(rgb, normal, depth, seg)
        self._check(self._c_render_color(self.h, camera_array(cams), len(cams), int(height), int(width), env_index, int(n_render),
                                         *(() if source is None else (int(source),)), C.byref(shading_struct(shading)), geom_rgb,
                                         int(bool(rgb_per_env)), C.byref(out), stream), "render_color")

    def _tool_pose(self, tool, q, env_index, n, pos, mat, jac, stream):
        self._check(self._c_tool_pose(self.h, C.byref(tool_spec(tool)), q, env_index, int(n), pos, mat, jac, stream), "tool_pose")

    def _tool_ik(self, tool, cfg, target_pos, target_mat, q_init, env_index, n, q_out, residual, info, stream):
        self._check(self._c_tool_ik(self.h, C.byref(tool_spec(tool)), C.byref(cfg), target_pos, target_mat, q_init, env_index, int(n),
                                    q_out, residual, info, stream), "tool_ik")

    def _contacts(self, env_index, n, forces, pairs, out, stream):
        arr = geom_pair_array(pairs, self._WORDS) if pairs else None
        self._check(self._c_contacts(self.h, env_index, int(n), int(bool(forces)), arr, len(pairs) if pairs else 0, C.byref(out), stream), "contacts")

    def _proximity(self, env_index, n, q, pairs, max_dist, out, stream, q_adr=()):
        """q_adr: () on the SO100 engine; on the tree engine (int32 array of the qpos addresses of q's columns or None, their count)"""
        arr = geom_pair_array(pairs, self._WORDS) if pairs else None
        self._check(self._c_proximity(self.h, env_index, int(n), q, *q_adr, arr, len(pairs) if pairs else 0, float(max_dist), C.byref(out), stream),
                    "proximity")


class Sim(_Handle):
    """Thin handle wrapper. All array arguments are raw device addresses (ints)."""

    def __init__(self, blob_f32: bytes, n_envs: int, device: int = 0, seed: int = 0, lib_path: str | None = None):
        self._create(lib_path, blob_f32, n_envs, int(device), int(seed))
        self.cfg = Config()
        self._c_default_config(C.byref(self.cfg))

    def configure(self, **kw):
        for k, v in kw.items():
            if k == "action_offset":
                for i in range(ACT_DIM):
                    self.cfg.action_offset[i] = float(v[i])
            else:
                if not hasattr(self.cfg, k):
                    raise AttributeError(k)
                setattr(self.cfg, k, v)
        self._check(self._c_configure(self.h, C.byref(self.cfg)), "configure")

    def info(self, stream=0) -> dict:
        """Facts about the handle (so101_get_info): which step path ran, graph replay, scheduler aborts, scratch size."""
        return {k: int(self._c_get_info(self.h, v, C.c_void_p(stream))) for k, v in INFO.items()}

    def chain_stats(self, clear=True, stream=0) -> dict:
        """Time accounting of the chained step's persistent kernel (so101_debug_chain_stats), seconds summed over wavefronts."""
        buf = (C.c_uint64 * 16)()
        self._check(self._c_debug_chain_stats(self.h, C.cast(buf, C.c_void_p), int(clear), C.c_void_p(stream)), "debug_chain_stats")
        k = ("t_pop", "t_idle", "t_narrow", "t_solve", "n_narrow", "n_solve", "n_idle", "waves", "t_life",
             "t_narrow_load", "t_narrow_pairs", "t_narrow_finish", "t_solve_load_gather", "t_solve_compute", "t_solve_store_broad", "t_solve_publish")
        d = {n: int(buf[i]) for i, n in enumerate(k)}
        for n in k:
            if not n.startswith("t_"):
                continue
            d[n] *= 1e-8
        return d

    def bind(self, qpos, qvel, ctrl, warmstart, obs_ring, ep_return, step_count, episode, mass_scale=None):
        b = Buffers(qpos, qvel, ctrl, warmstart, obs_ring, ep_return, step_count, episode, mass_scale)
        self._check(self._c_bind_state(self.h, C.byref(b)), "bind_state")

    def set_reset_pool(self, qpos, qvel, ctrl, pool_size: int):
        self._check(self._c_set_reset_pool(self.h, qpos, qvel, ctrl, int(pool_size)), "set_reset_pool")

    def compute_settled(self, first_episode: int, n_episodes: int, qpos, qvel, warm, flags, stream=0):
        self._check(self._c_compute_settled(self.h, int(first_episode), int(n_episodes), qpos, qvel, warm, flags, stream), "compute_settled")

    def set_settled_store(self, qpos, qvel, warm, flags, first_episode: int, n_episodes: int):
        self._check(self._c_set_settled_store(self.h, qpos, qvel, warm, flags, int(first_episode), int(n_episodes)), "set_settled_store")

    def reset(self, mask=None, stream=0):
        self._check(self._c_reset(self.h, mask, stream), "reset")

    def settle(self, stream=0):
        self._check(self._c_settle(self.h, stream), "settle")

    def begin_episode(self, stream=0):
        self._check(self._c_begin_episode(self.h, stream), "begin_episode")

    def step(self, action, obs, reward, discount, step_type, stream=0):
        self._check(self._c_step(self.h, action, obs, reward, discount, step_type, stream), "step")

    def physics(self, n_substeps: int, freeze_arm: bool = False, stream=0):
        self._check(self._c_physics(self.h, int(n_substeps), int(freeze_arm), stream), "physics")

    def reward(self, out, stream=0):
        self._check(self._c_reward(self.h, out, stream), "reward")

    def get_returns(self, out, stream=0):
        self._check(self._c_get_returns(self.h, out, stream), "get_returns")

    def get_diag(self, out, stream=0):
        self._check(self._c_get_diag(self.h, out, stream), "get_diag")

    def get_events(self, out, clear=False, stream=0):
        self._check(self._c_get_events(self.h, out, int(bool(clear)), stream), "get_events")

    def debug_candidates(self, ncand=None, cand=None, ticks=None, conres=None, stream=0):
        self._check(self._c_debug_candidates(self.h, ncand, cand, ticks, conres, stream), "debug_candidates")

    def debug_stages(self, out, stream=0):
        self._check(self._c_debug_stages(self.h, out, stream), "debug_stages")

    def debug_forward(self, out, stream=0):
        self._check(self._c_debug_forward(self.h, out, stream), "debug_forward")

    def set_hull_planes(self, planes, plane_adr):
        """planes [n, 4] float32 and plane_adr [ngeom + 1] int32: HOST numpy arrays (so101_set_hull_planes copies them)"""
        self._set_hull_planes(planes, plane_adr)

    def render(self, cams, height: int, width: int, env_index, n_render: int, depth, seg, stream=0):
        """cams: sequence of (body, pos[3], mat[9] row-major, fovy_deg); env_index / depth / seg: raw device addresses or None"""
        self._render(cams, height, width, env_index, n_render, depth, seg, stream)

    def render_color(self, cams, height: int, width: int, env_index, n_render: int, shading, geom_rgb, rgb_per_env: bool = False,
                     rgb=None, normal=None, depth=None, seg=None, stream=0):
        """so101_render_color.  cams as for render; shading: what shading_struct() takes; geom_rgb / env_index / rgb / normal / depth / seg: raw
        device addresses or None (geom_rgb [ngeom, 3] float32, or [n_envs, ngeom, 3] with rgb_per_env)"""
        self._render_color(cams, height, width, env_index, n_render, shading, geom_rgb, rgb_per_env, rgb, normal, depth, seg, stream)

    def ik_config(self, **kw) -> IkConfig:
        """so101_ik_default_config (mode 1, 60 iterations, 1e-4 m, 1e-3 rad, the model's joint ranges) with the given fields replaced;
        q_lo / q_hi take sequences of 6"""
        cfg = IkConfig()
        self._check(self._c_ik_default_config(self.h, C.byref(cfg)), "ik_default_config")
        for k, v in kw.items():
            if k in ("q_lo", "q_hi"):
                getattr(cfg, k)[:] = [float(x) for x in v]
            elif hasattr(cfg, k):
                setattr(cfg, k, v)
            else:
                raise TypeError(f"unknown IK setting {k!r}")
        return cfg

    def tool_pose(self, tool, q, env_index, n: int, pos, mat, jac, stream=0):
        """tool: (body, pos[3], mat[9] row-major); q / env_index / pos / mat / jac: raw device addresses or None (so101_tool_pose)"""
        self._tool_pose(tool, q, env_index, n, pos, mat, jac, stream)

    def tool_ik(self, tool, cfg: IkConfig, target_pos, target_mat, q_init, env_index, n: int, q_out, residual, info, stream=0):
        """so101_tool_ik; cfg from ik_config(); the arrays are raw device addresses or None"""
        self._tool_ik(tool, cfg, target_pos, target_mat, q_init, env_index, n, q_out, residual, info, stream)

    def contacts(self, env_index, n: int, forces: bool, pairs, out: ContactOut, stream=0):
        """so101_contacts; pairs: sequence of (a words[4], b words[4]) geom masks; env_index and the fields of `out`: raw device addresses or None"""
        self._contacts(env_index, n, forces, pairs, out, stream)

    def proximity(self, env_index, n: int, q, pairs, max_dist: float, out: ProximityOut, stream=0):
        """so101_proximity; pairs: sequence of (a words[4], b words[4]) geom masks; env_index, q and the fields of `out`: raw device addresses or None"""
        self._proximity(env_index, n, q, pairs, max_dist, out, stream)


class TreeSim(_Handle):
    """Handle of the general-tree engine (include/so101.h, so101_tree_*): the ALOHA scenes.  Array arguments are raw device
    addresses (ints), state arrays are [dim][n_envs] float32."""
    _PREFIX = "so101_tree_"
    _WORDS = 8

    def __init__(self, blob_f32: bytes, n_envs: int, device: int = 0, lib_path: str | None = None):
        self._create(lib_path, blob_f32, n_envs, int(device))
        d = (C.c_int * 16)()
        self._check(self._c_dims(self.h, d), "dims")
        self.nq, self.nv, self.nu, self.nbody, self.ngeom, self.debug_dim, self.max_contacts = list(d)[:7]
        # layout of so101_tree_debug_forward's row for this handle's build (32 or 64 dofs) and the build itself
        self.dbg = dict(COUNTS=0, BIAS=d[7], QSM=d[8], QACC=d[9], XPOS=d[10], M=d[11], CON=d[12], FORCE=d[13], MSTRIDE=d[14])
        self.build = int(d[15])
        self.obs_dim = int(self._c_obs_dim(self.h))
        self.cfg = TreeConfig(n_substeps=10, last_step=1 << 30, settle_max_substeps=1000, terminate_on_success=1, solver_iterations=0,
                              solver_tolerance=-1.0, seed=0, env_id_base=0, reward_mode=0, reward_requires_handover=0,
                              joints_delay_steps=-1, physics_delay_steps=-1, prefetch_resets=0, pipeline=0)

    def bind(self, qpos, qvel, ctrl, warm):
        self._check(self._c_bind_state(self.h, qpos, qvel, ctrl, warm), "bind_state")

    def configure(self, solver_iterations: int = 0, solver_tolerance: float = -1.0):
        self._check(self._c_configure(self.h, int(solver_iterations), float(solver_tolerance)), "configure")

    def physics(self, n_substeps: int, stream: int = 0):
        self._check(self._c_physics(self.h, int(n_substeps), stream), "physics")

    def debug_forward(self, out, stream: int = 0):
        self._check(self._c_debug_forward(self.h, out, stream), "debug_forward")

    def get_diag(self, out, stream: int = 0):
        self._check(self._c_get_diag(self.h, out, stream), "get_diag")

    def bind_env(self, ring_pos, ring_vel, ep_return, step_count, episode):
        self._check(self._c_bind_env(self.h, ring_pos, ring_vel, ep_return, step_count, episode), "bind_env")

    def configure_env(self, **kw):
        for k, v in kw.items():
            if not hasattr(self.cfg, k):
                raise TypeError(f"unknown config field {k}")
            setattr(self.cfg, k, v)
        self._check(self._c_configure_env(self.h, C.byref(self.cfg)), "configure_env")

    def reset(self, mask=None, stream: int = 0):
        self._check(self._c_reset(self.h, mask, stream), "reset")

    def last_plan(self):
        """(env slices, kernel launches, memsets, path) of the last so101_tree_step as the library enqueued it; path 0 = no step yet"""
        d = (C.c_int * 4)()
        self._check(self._c_last_plan(self.h, d), "last_plan")
        return tuple(d)

    def step(self, action, obs, reward, discount, step_type, stream: int = 0):
        self._check(self._c_step(self.h, action, obs, reward, discount, step_type, stream), "step")

    def begin_episode(self, stream: int = 0):
        self._check(self._c_begin_episode(self.h, stream), "begin_episode")

    def settle(self, stream: int = 0):
        self._check(self._c_settle(self.h, stream), "settle")

    def compute_settled(self, first_episode, count, qpos, qvel, warm, flags, stream: int = 0):
        self._check(self._c_compute_settled(self.h, int(first_episode), int(count), qpos, qvel, warm, flags, stream), "compute_settled")

    def set_settled_store(self, first_episode, count, qpos, qvel, warm, flags):
        self._check(self._c_set_settled_store(self.h, int(first_episode), int(count), qpos, qvel, warm, flags), "set_settled_store")

    def set_hull_planes(self, planes, plane_adr):
        """planes [n, 4] float32 and plane_adr [ngeom + 1] int32: HOST numpy arrays (so101_tree_set_hull_planes copies them)"""
        self._set_hull_planes(planes, plane_adr)

    def render(self, cams, height: int, width: int, env_index, n_render: int, depth, seg, stream=0, source: int = 0):
        """cams: sequence of (body, pos[3], mat[9] row-major, fovy_deg), body a tree body id (-1 or 0: the world); env_index / depth / seg: raw
        device addresses or None; source 0: the bound qpos, 1: the delayed physics-state line (so101_tree_bind_physics_state)"""
        self._render(cams, height, width, env_index, n_render, depth, seg, stream, source=source)

    def render_color(self, cams, height: int, width: int, env_index, n_render: int, shading, geom_rgb, rgb_per_env: bool = False,
                     rgb=None, normal=None, depth=None, seg=None, stream=0, source: int = 0):
        """so101_tree_render_color: native.Sim.render_color on this engine; cams and source as for render"""
        self._render_color(cams, height, width, env_index, n_render, shading, geom_rgb, rgb_per_env, rgb, normal, depth, seg, stream, source=source)

    def tool_chain(self, body: int):
        """The columns of a tool on body `body` (so101_tree_tool_chain): (dof indices, qpos addresses, joint types 1 hinge / 3 slide), root first"""
        dof, qadr, jt = ((C.c_int32 * TREE_TOOL_MAXCOL)() for _ in range(3))
        n = self._c_tool_chain(self.h, int(body), dof, qadr, jt)
        if n < 0:
            self._check(n, "tool_chain")
        return list(dof[:n]), list(qadr[:n]), list(jt[:n])

    def ik_config(self, body: int, **kw) -> TreeIkConfig:
        """so101_tree_ik_default_config for a tool on `body` (mode 1, 60 iterations, 1e-4 m, 1e-3 rad, the chain's joint ranges, the hinge columns
        free) with the given fields replaced; q_lo / q_hi take one value per column of the chain"""
        cfg = TreeIkConfig()
        self._check(self._c_ik_default_config(self.h, int(body), C.byref(cfg)), "ik_default_config")
        for k, v in kw.items():
            if k in ("q_lo", "q_hi"):
                v = [float(x) for x in v]
                if len(v) > TREE_TOOL_MAXCOL:
                    raise ValueError(f"{k} takes at most {TREE_TOOL_MAXCOL} values")
                getattr(cfg, k)[:len(v)] = v
            elif hasattr(cfg, k):
                setattr(cfg, k, v)
            else:
                raise TypeError(f"unknown IK setting {k!r}")
        return cfg

    def tool_pose(self, tool, q, env_index, n: int, pos, mat, jac, stream=0):
        """tool: (body id, pos[3], mat[9] row-major); q / env_index / pos / mat / jac: raw device addresses or None (so101_tree_tool_pose)"""
        self._tool_pose(tool, q, env_index, n, pos, mat, jac, stream)

    def tool_ik(self, tool, cfg: TreeIkConfig, target_pos, target_mat, q_init, env_index, n: int, q_out, residual, info, stream=0):
        """so101_tree_tool_ik; cfg from ik_config(); the arrays are raw device addresses or None"""
        self._tool_ik(tool, cfg, target_pos, target_mat, q_init, env_index, n, q_out, residual, info, stream)

    def contacts(self, env_index, n: int, forces: bool, pairs, out: ContactOut, stream=0):
        """so101_tree_contacts; pairs: sequence of (a words[8], b words[8]) geom masks; env_index and the fields of `out`: raw device addresses or
        None.  The per-contact fields of `out` have max_contacts slots per entry."""
        self._contacts(env_index, n, forces, pairs, out, stream)

    def proximity(self, env_index, n: int, q, q_adr, pairs, max_dist: float, out: ProximityOut, stream=0):
        """so101_tree_proximity; pairs: sequence of (a words[8], b words[8]) geom masks; q_adr: the qpos addresses of q's columns (a sequence of
        ints, host side) or None; env_index, q [n][len(q_adr)] and the fields of `out`: raw device addresses or None"""
        adr = (C.c_int32 * len(q_adr))(*[int(a) for a in q_adr]) if q_adr is not None and len(q_adr) else None
        self._proximity(env_index, n, q, pairs, max_dist, out, stream, q_adr=(adr, len(q_adr) if q_adr is not None else 0))


