"""Shared inputs of the Cartesian tool tests (test_tool_emu.py on the emulated build, test_tool_gpu.py on the MI355X): the tools, the
seeded IK cases with their fp64 targets, and one so101_tool_pose / so101_tool_ik call through tests/simharness.ArraySim.

An IK case: q_target = lo + (0.05 + 0.9 u)(hi - lo), the target is FK(q_target), q_init = clamp(q_target + 0.3 (2 u - 1), lo, hi), with
lo, hi the blob's jnt_range and u drawn from RandomState(seed) case by case (six numbers for the target, then six for the start).  Every
case is solvable by construction and the start is at most 0.3 rad per joint away; test_tool_emu.py asserts that the fp64 reference converges on all of them in every mode within 10 iterations."""
from __future__ import annotations

import functools

import numpy as np

from so101_sim_amd import tools
from so101_sim_amd.model import blob as blobfmt, scenes
from tests.tool_ref import ToolRef

N_CASES = 512
IDENTITY_TOOL = tools.Tool("link0", 0)
# a tool on the moving jaw (link 5), off its origin and rotated: every column of the Jacobian is in use
JAW_TOOL = tools.Tool.from_xyaxes("moving_jaw_tip", 5, (0.004, -0.03, 0.012), (0.6, 0.8, 0.0, -0.32, 0.24, 0.92))
# a tool on an inner link (link 2): three walked columns, and three trailing joints that the IK clamps and hands back
INNER_TOOL = tools.Tool.from_xyaxes("lower_arm_point", 2, (0.02, -0.09, 0.015), (0.0, 0.6, 0.8, 1.0, 0.0, 0.0))
N_INNER, INNER_SEED = 65, 3


@functools.lru_cache(maxsize=None)
def reference() -> ToolRef:
    return ToolRef(scenes.load_blob("banana", "f64")[0])


@functools.lru_cache(maxsize=None)
def pad_tool() -> tools.Tool:
    raw, meta = scenes.load_blob("banana", "f64")
    return tools.so100_tools(meta, blobfmt.unpack(raw))[tools.DEFAULT_TOOL]


def spec(tool):
    """a tools.Tool as the (body, pos, mat [3, 3]) tuple tests/tool_ref.py takes"""
    return tool.body, np.asarray(tool.pos, dtype=np.float64), np.asarray(tool.mat, dtype=np.float64).reshape(3, 3)


@functools.lru_cache(maxsize=None)
def _cases(seed: int):
    ref, tool = reference(), pad_tool()
    rs = np.random.RandomState(seed)
    lo, hi = ref.lo, ref.hi
    u = rs.uniform(size=(N_CASES, 2, 6))              # case by case: six draws for the target, then six for the start
    q_target = lo + (0.05 + 0.9 * u[:, 0]) * (hi - lo)
    q_init = np.clip(q_target + 0.3 * (2.0 * u[:, 1] - 1.0), lo, hi)
    pos, mat = np.zeros((N_CASES, 3)), np.zeros((N_CASES, 3, 3))
    for i in range(N_CASES):
        pos[i], mat[i], _ = ref.fk(q_target[i], spec(tool), jacobian=False)
    out = dict(q_target=q_target, q_init=q_init, pos=pos, mat=mat)
    for a in out.values():
        a.setflags(write=False)
    return out


def ik_cases(seed: int):
    """the cases of the scene's own tool (fixed_jaw_pad): dict of read-only arrays q_target [512, 6], q_init [512, 6], pos [512, 3], mat [512, 3, 3],
    computed once per seed"""
    return _cases(int(seed))


@functools.lru_cache(maxsize=None)
def inner_cases(seed: int = INNER_SEED):
    """65 position-only cases of INNER_TOOL: dict of read-only arrays pos [65, 3] = FK of joints drawn over their whole range (the first three
    move the tool) and q_init [65, 6] within the range: the three joints beyond the tool's link over all of it, the three walked ones within
    1 rad of the target's.  Position-only damped least squares with clamping stalls at a joint limit on the wrong branch of the arm for 31 % of
    starts drawn over the whole range (200 draws, whatever the tool's offset), 1 % at 1 rad: from there about every second seed gives 65
    solvable cases.  test_tool_emu.py asserts that the fp64 reference converges on all of them within the default 60 iterations."""
    ref = reference()
    u = np.random.RandomState(seed).uniform(size=(2, N_INNER, 6))
    q_target, q_init = ref.lo + u[0] * (ref.hi - ref.lo), ref.lo + u[1] * (ref.hi - ref.lo)
    q_init[:, :3] = np.clip(q_target[:, :3] + 1.0 * (2.0 * u[1, :, :3] - 1.0), ref.lo[:3], ref.hi[:3])
    pos = np.array([ref.fk(q, spec(INNER_TOOL), jacobian=False)[0] for q in q_target])
    out = dict(q_init=q_init, pos=pos)
    for a in out.values():
        a.setflags(write=False)
    return out


def check_inner_link(sim, n):
    """so101_tool_ik (mode 0) and so101_tool_pose for the first n inner-link cases on an ArraySim of either backend: every solve converges, the
    reported residual is the fp64 one of q_out within the margins of tests/test_tool_gpu.py (2e-6 m, 1e-5 rad), the joints beyond the tool's
    link come back as clip(q_init) bit for bit, and their Jacobian columns are +0."""
    ref, cs = reference(), inner_cases()
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)
    q, res, info = tool_ik(sim, INNER_TOOL, cs["pos"][:n], None, cs["q_init"][:n], mode=0)
    print(f"inner-link IK, n = {n}: iterations {info.tolist()}")
    assert np.all(info >= 0), np.flatnonzero(info < 0)
    worst = np.zeros(2)
    for i in range(n):
        rp, rr_ = ref.residual(q[i], spec(INNER_TOOL), cs["pos"][i], None, 0)
        worst = np.maximum(worst, [abs(res[i, 0] - rp), abs(res[i, 1] - rr_)])
    print(f"inner-link IK, n = {n}: reported - fp64 residual worst {worst[0]:.3e} m {worst[1]:.3e} rad")
    assert worst[0] <= 2e-6 and worst[1] <= 1e-5
    held = np.clip(cs["q_init"][:n, 3:].astype(np.float32), ref.lo[3:].astype(np.float32), ref.hi[3:].astype(np.float32))
    assert np.array_equal(bits(q[:, 3:]), bits(held))
    _, _, jac = tool_pose(sim, INNER_TOOL, n, q=q)
    assert np.all(bits(jac[:, :, 3:]) == 0) and np.any(jac[:, :, :3] != 0)


def random_q(seed: int, n: int):
    ref = reference()
    return ref.lo + np.random.RandomState(seed).uniform(size=(n, 6)) * (ref.hi - ref.lo)


def _dev(sim, a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return sim.torch.as_tensor(a).to(sim.dev) if sim.backend == "gpu" else a


def _out(sim, shape, dtype, fill):
    if sim.backend == "gpu":
        t = sim.torch
        return t.full(shape, fill, dtype=t.float32 if dtype == np.float32 else t.int32, device=sim.dev)
    return np.full(shape, fill, dtype=dtype)


def tool_pose(sim, tool, n, q=None, env_index=None, jacobian=True):
    """so101_tool_pose on an ArraySim (either backend) -> numpy pos [n, 3], mat [n, 3, 3], jac [n, 6, 6] (float32).  The outputs start
    as 7e7, so an entry the kernel does not write fails every check."""
    qd = None if q is None else _dev(sim, np.asarray(q).reshape(n, 6), np.float32)
    idx = None if env_index is None else _dev(sim, env_index, np.int32)
    pos, mat = _out(sim, (n, 3), np.float32, 7e7), _out(sim, (n, 3, 3), np.float32, 7e7)
    jac = _out(sim, (n, 6, 6), np.float32, 7e7) if jacobian else None
    p = lambda a: None if a is None else sim.ptr(a)
    sim.sim.tool_pose(tool.spec(), p(qd), p(idx), n, p(pos), p(mat), p(jac), sim.stream())
    return sim._get(pos), sim._get(mat), (sim._get(jac) if jacobian else None)


def tool_ik(sim, tool, target_pos, target_mat, q_init=None, env_index=None, **cfg):
    """so101_tool_ik on an ArraySim -> numpy q_out [n, 6] float32, residual [n, 2] float32, info [n] int32"""
    n = len(target_pos)
    tp = _dev(sim, np.asarray(target_pos).reshape(n, 3), np.float32)
    tm = None if target_mat is None else _dev(sim, np.asarray(target_mat).reshape(n, 9), np.float32)
    qi = None if q_init is None else _dev(sim, np.asarray(q_init).reshape(n, 6), np.float32)
    idx = None if env_index is None else _dev(sim, env_index, np.int32)
    q, res, info = _out(sim, (n, 6), np.float32, 7e7), _out(sim, (n, 2), np.float32, 7e7), _out(sim, (n,), np.int32, -7)
    p = lambda a: None if a is None else sim.ptr(a)
    sim.sim.tool_ik(tool.spec(), sim.sim.ik_config(**cfg), p(tp), p(tm), p(qi), p(idx), n, p(q), p(res), p(info), sim.stream())
    return sim._get(q), sim._get(res), sim._get(info)
