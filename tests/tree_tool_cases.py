"""Shared inputs of the tree engine's Cartesian tool tests (test_tree_tool_emu.py on the emulated build, test_tree_tool_gpu.py on the MI355X):
the tools, the default limits, the seeded IK cases with their fp64 targets, and one so101_tree_tool_pose / so101_tree_tool_ik call through
tests/simharness.TreeArraySim.

An IK case of a tool with ncol columns and limits lo, hi (the default limits of the Python layer: the blob's jnt_range intersected with
aloha_action_spec on the actuated arm joints, restated here from the blob): q_target = lo + (0.05 + 0.9 u)(hi - lo), the target is
FK(q_target), q_init = clamp(q_target + 0.3 (2 u - 1), lo, hi) on the free columns (the hinges) and q_target on the held ones (a finger's
slide), with u drawn from RandomState(seed) case by case (ncol numbers for the target, then ncol for the start).  Every case is solvable by
construction; test_tree_tool_emu.py asserts that the fp64 reference converges on all of them in every mode."""
from __future__ import annotations

import functools

import numpy as np

from so101_sim_amd import aloha, tools
from so101_sim_amd.model import blob as blobfmt
from tests import tree_render_cases as trc
from tests.tree_tool_ref import TreeToolRef

N_CASES = 512
# a tool on the right arm's left finger, off its origin and rotated: 7 columns, the last one a slide
FINGER_TOOL = tools.Tool.from_xyaxes("right_finger_tip", "right/left_finger_link", (0.012, -0.05, 0.018), (0.6, 0.8, 0.0, -0.32, 0.24, 0.92))
# a tool two joints up the left arm: 2 columns
UPPER_TOOL = tools.Tool.from_xyaxes("left_upper_arm", "left/upper_arm_link", (0.05, 0.0, 0.2))
TOOLS = ("left/gripper", "right/gripper", FINGER_TOOL, UPPER_TOOL)


@functools.lru_cache(maxsize=None)
def reference(scene: str = "banana") -> TreeToolRef:
    return TreeToolRef(trc.blobs(scene)["f64"])


def resolved(tool, scene: str = "banana") -> tools.Tool:
    """a name of tools.ALOHA_TOOLS or a Tool, its body resolved against the scene's body names"""
    return tools.resolve(tool, tools.ALOHA_TOOLS).with_body_ids(trc.blobs(scene)["meta"]["body_names"])


def spec(tool, scene: str = "banana"):
    """a tool as the (body, pos, mat [3, 3]) tuple tests/tree_tool_ref.py takes"""
    t = resolved(tool, scene)
    return t.body, np.asarray(t.pos, dtype=np.float64), np.asarray(t.mat, dtype=np.float64).reshape(3, 3)


@functools.lru_cache(maxsize=None)
def _limits(body: int, scene: str):
    ref = reference(scene)
    m = blobfmt.unpack(trc.blobs(scene)["f32"])
    lo, hi = ref.limits(body)
    lo, hi = lo.astype(np.float32).astype(np.float64), hi.astype(np.float32).astype(np.float64)          # (the library holds them in float32)
    act = aloha.aloha_action_spec(np.asarray(m["act_ctrlrange"], dtype=np.float64).reshape(-1, 2))
    grip, adof = np.asarray(m["task_act_is_gripper"]).ravel(), [int(d) for d in np.asarray(m["act_dof"]).ravel()]
    for k, d in enumerate(ref.columns(body)[0]):
        if d in adof and not int(grip[adof.index(d)]):
            a = adof.index(d)
            lo[k], hi[k] = max(lo[k], float(act.minimum[a])), min(hi[k], float(act.maximum[a]))
    lo.setflags(write=False); hi.setflags(write=False)
    return lo, hi


def limits(tool, scene: str = "banana"):
    """default limits of the Python layer for the tool's chain: (lo [ncol], hi [ncol]) float64 holding float32 values"""
    return _limits(resolved(tool, scene).body, scene)


@functools.lru_cache(maxsize=None)
def _cases(tool_key, seed: int):
    tool = TOOLS[tool_key]
    ref, sp = reference(), spec(tool)
    lo, hi = limits(tool)
    ncol = len(lo)
    free = np.array([(ref.hinge_mask(sp[0]) >> k) & 1 for k in range(ncol)], dtype=bool)
    u = np.random.RandomState(seed).uniform(size=(N_CASES, 2, ncol))
    q_target = lo + (0.05 + 0.9 * u[:, 0]) * (hi - lo)
    q_init = np.where(free, np.clip(q_target + 0.3 * (2.0 * u[:, 1] - 1.0), lo, hi), q_target)
    pos, mat = np.zeros((N_CASES, 3)), np.zeros((N_CASES, 3, 3))
    for i in range(N_CASES):
        pos[i], mat[i], _ = ref.fk(q_target[i], sp, jacobian=False)
    out = dict(q_target=q_target, q_init=q_init, pos=pos, mat=mat)
    for a in out.values():
        a.setflags(write=False)
    return out


def ik_cases(tool, seed: int):
    """the cases of one of TOOLS: dict of read-only arrays q_target [512, ncol], q_init [512, ncol], pos [512, 3], mat [512, 3, 3], computed once"""
    return _cases(TOOLS.index(tool), int(seed))


def random_q(tool, seed: int, n: int, scene: str = "banana"):
    lo, hi = limits(tool, scene)
    return lo + np.random.RandomState(seed).uniform(size=(n, len(lo))) * (hi - lo)


def _dev(sim, a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return sim.torch.as_tensor(a).to(sim.dev) if sim.backend == "gpu" else a


def _out(sim, shape, dtype, fill):
    if sim.backend == "gpu":
        t = sim.torch
        return t.full(shape, fill, dtype=t.float32 if dtype == np.float32 else t.int32, device=sim.dev)
    return np.full(shape, fill, dtype=dtype)


PAD, FILL = 5, 7e7          # floats past the end of every output, and what the outputs start as


def _padded(sim, a, count, what):
    """the first `count` values of a flat output; what lies beyond must still be the fill: nothing is written there"""
    a = sim._get(a)
    assert np.all(a[count:] == a.dtype.type(FILL if a.dtype == np.float32 else -7)), f"{what}: written past its end"
    return a[:count]


def tool_pose(sim, tool, n, q=None, env_index=None, jacobian=True, scene: str = "banana"):
    """so101_tree_tool_pose on a TreeArraySim (either backend) -> numpy pos [n, 3], mat [n, 3, 3], jac [n, 6, ncol] (float32).  The outputs
    start as 7e7, so an entry the kernel does not write fails every check; each has a few floats of padding that must stay untouched (a
    kernel that wrote columns the chain does not have - 8 per row instead of ncol - would run into it)."""
    t = resolved(tool, scene)
    ncol = len(sim.sim.tool_chain(t.body)[0])
    qd = None if q is None else _dev(sim, np.asarray(q).reshape(n, ncol), np.float32)
    idx = None if env_index is None else _dev(sim, env_index, np.int32)
    pos, mat = _out(sim, (n * 3 + PAD,), np.float32, FILL), _out(sim, (n * 9 + PAD,), np.float32, FILL)
    jac = _out(sim, (n * 6 * ncol + PAD,), np.float32, FILL) if jacobian else None
    p = lambda a: None if a is None else sim.ptr(a)
    sim.sim.tool_pose(t.spec(), p(qd), p(idx), n, p(pos), p(mat), p(jac), sim.stream())
    return (_padded(sim, pos, n * 3, "pos").reshape(n, 3), _padded(sim, mat, n * 9, "mat").reshape(n, 3, 3),
            _padded(sim, jac, n * 6 * ncol, "jac").reshape(n, 6, ncol) if jacobian else None)


def tool_ik(sim, tool, target_pos, target_mat, q_init=None, env_index=None, scene: str = "banana", **cfg):
    """so101_tree_tool_ik on a TreeArraySim -> numpy q_out [n, ncol] float32, residual [n, 2] float32, info [n] int32; the limits default
    to limits(tool)"""
    t = resolved(tool, scene)
    ncol = len(sim.sim.tool_chain(t.body)[0])
    n = len(target_pos)
    lo, hi = limits(tool, scene)
    cfg = dict(dict(q_lo=lo, q_hi=hi), **cfg)
    tp = _dev(sim, np.asarray(target_pos).reshape(n, 3), np.float32)
    tm = None if target_mat is None else _dev(sim, np.asarray(target_mat).reshape(n, 9), np.float32)
    qi = None if q_init is None else _dev(sim, np.asarray(q_init).reshape(n, ncol), np.float32)
    idx = None if env_index is None else _dev(sim, env_index, np.int32)
    q, res, info = _out(sim, (n * ncol + PAD,), np.float32, FILL), _out(sim, (n * 2 + PAD,), np.float32, FILL), _out(sim, (n + PAD,), np.int32, -7)
    p = lambda a: None if a is None else sim.ptr(a)
    sim.sim.tool_ik(t.spec(), sim.sim.ik_config(t.body, **cfg), p(tp), p(tm), p(qi), p(idx), n, p(q), p(res), p(info), sim.stream())
    return _padded(sim, q, n * ncol, "q_out").reshape(n, ncol), _padded(sim, res, n * 2, "residual").reshape(n, 2), _padded(sim, info, n, "info")
