"""Cartesian tool control of the general-tree engine without a GPU: self-checks of the fp64 reference (tests/tree_tool_ref.py), solvability of
the shared IK cases (tests/tree_tool_cases.py), the tool table, and the library's chains, argument checks, pose, Jacobian and IK through the
emulated build of the kernel source (tests/hostemu), on both builds of the engine."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from so101_sim_amd import native, tools
from tests import tree_render_cases as trc, tree_tool_cases as tc
from tests.simharness import TreeArraySim

# float32 bounds of the pose test (tests/test_tree_tool_gpu.py states where they come from)
POS_TOL, MAT_TOL, JAC_TOL = 3.4e-6, 5.1e-6, 4.9e-6
RES_POS, RES_ROT = POS_TOL, 2 * MAT_TOL
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aloha_sites.json")
HINGE, SLIDE = native.TREE_JNT_HINGE, native.TREE_JNT_SLIDE


def test_aloha_tool_table_matches_the_reference_sites():
    sites = json.load(open(GOLDEN))["sites"]
    assert {s["name"] for s in sites} == set(tools.ALOHA_TOOLS) and len(sites) == 6
    for s in sites:
        t = tools.ALOHA_TOOLS[s["name"]]
        assert t.body == s["body"] and t.name == s["name"]
        np.testing.assert_array_equal(t.pos, s["pos"] if s["pos"] is not None else (0.0, 0.0, 0.0))
        want = np.eye(3) if s["quat"] is None else tools.frame_from_quat(s["quat"])
        np.testing.assert_allclose(np.array(t.mat), want, atol=1e-15)
    g = tools.ALOHA_TOOLS["left/gripper"]
    assert g.body == "left/gripper_link" and g.pos == (0.15, 0.0, 0.0) and tools.ALOHA_TOOLS["right/gripper"].body == "right/gripper_link"
    names = trc.blobs("banana")["meta"]["body_names"]
    assert g.with_body_ids(names).body == names.index("left/gripper_link")
    with pytest.raises(ValueError, match="is a name"):
        g.spec()
    with pytest.raises(ValueError, match="no body"):
        tools.Tool("t", "no/such_link").with_body_ids(names)
    with pytest.raises(ValueError, match="unknown tool"):
        tools.resolve("gripper", tools.ALOHA_TOOLS)
    assert tools.Tool("t", 3).with_body_ids(names).body == 3


def test_reference_pose_equals_the_camera_reference():
    worst = 0.0
    for scene, states in (("banana", [trc.STATES[k] for k in trc.STATE_NAMES]), ("dining", [trc.DINING_STATE])):
        ref = tc.reference(scene)
        for tool in tc.TOOLS:
            body, pos, mat = tc.spec(tool, scene)
            for qpos in states:
                p, M, _ = ref.fk_qpos(qpos, (body, pos, mat), jacobian=False)
                cp, cM = ref.camera_frame(qpos, (body, pos, mat, 45.0))
                worst = max(worst, np.abs(p - cp).max(), np.abs(M - cM).max())
                # the chain's joints alone fix the pose: the other entries of qpos do not move the tool
                q = [qpos[a] for a in ref.columns(body)[1]]
                p2, M2, _ = ref.fk(q, (body, pos, mat), jacobian=False)
                worst = max(worst, np.abs(p2 - cp).max(), np.abs(M2 - cM).max())
    print(f"tree tool reference vs camera reference: worst difference {worst:.3e}")
    assert worst <= 1e-12


def test_reference_jacobian_matches_central_differences():
    ref = tc.reference()
    h, worst = 1e-6, 0.0
    for tool in tc.TOOLS:
        sp = tc.spec(tool)
        types = ref.columns(sp[0])[2]
        for q in tc.random_q(tool, 4, 6):
            _, M, J = ref.fk(q, sp)
            assert J.shape == (6, len(types))
            for j in range(len(types)):
                d = np.zeros(len(types)); d[j] = h
                pp, Mp, _ = ref.fk(q + d, sp, jacobian=False)
                pm, Mm, _ = ref.fk(q - d, sp, jacobian=False)
                W = (Mp - Mm) @ M.T / (2 * h)              # skew matrix of the angular velocity per unit joint rate
                num = np.r_[(pp - pm) / (2 * h), W[2, 1], W[0, 2], W[1, 0]]
                worst = max(worst, np.abs(num - J[:, j]).max())
                if types[j] == SLIDE:
                    assert np.all(J[3:, j] == 0) and abs(np.linalg.norm(J[:3, j]) - 1) < 1e-12
    assert SLIDE in ref.columns(tc.spec(tc.FINGER_TOOL)[0])[2]
    print(f"analytic Jacobian vs central differences: worst difference {worst:.3e}")
    assert worst <= 1e-8


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("tool", [0, 1, 2])
def test_reference_ik_converges_on_every_shared_case(tool, seed):
    """a condition on the inputs of the device tests: all 512 cases of the seed, all three modes, at most 30 iterations in fp64, and at most
    10 on cases 0..129 (the ones the device tests use)"""
    tool = tc.TOOLS[tool]
    ref, sp, cs = tc.reference(), tc.spec(tool), tc.ik_cases(tool, seed)
    lo, hi = tc.limits(tool)
    held = [k for k, t in enumerate(ref.columns(sp[0])[2]) if t == SLIDE]
    for mode in (0, 1, 2):
        worst = worst130 = 0
        for i in range(tc.N_CASES):
            q, info, res = ref.ik(sp, cs["pos"][i], cs["mat"][i], cs["q_init"][i], lo=lo, hi=hi, mode=mode)
            assert 0 <= info <= (10 if i < 130 else 30), (seed, mode, i, info, res)
            assert np.all(q >= lo) and np.all(q <= hi) and np.all(q[held] == cs["q_init"][i][held])
            worst = max(worst, info)
            worst130 = max(worst130, info) if i < 130 else worst130
        print(f"fp64 IK, {tc.resolved(tool).name}, seed {seed}, mode {mode}: 512/512 converged, worst {worst} iterations, cases 0..129 worst {worst130}")


def test_tool_chains_of_both_builds():
    for scene in ("banana", "dining"):
        sim = TreeArraySim(trc.blobs(scene)["f32"], 1, backend="emu")
        assert sim.sim.build == (64 if scene == "dining" else 32)
        ref = tc.reference(scene)
        dof, qadr, jt = sim.sim.tool_chain(tc.resolved("left/gripper", scene).body)
        assert dof == [0, 1, 2, 3, 4, 5] and jt == [HINGE] * 6 and qadr == [0, 1, 2, 3, 4, 5]
        dof, qadr, jt = sim.sim.tool_chain(tc.resolved(tc.FINGER_TOOL, scene).body)
        assert dof == [8, 9, 10, 11, 12, 13, 14] and jt == [HINGE] * 6 + [SLIDE]
        for tool in tc.TOOLS:
            body = tc.resolved(tool, scene).body
            assert tuple(sim.sim.tool_chain(body)) == tuple(ref.columns(body))
        assert len(sim.sim.tool_chain(tc.resolved(tc.UPPER_TOOL, scene).body)[0]) == 2
        # the default configuration: the SO100 settings, the chain's jnt_range, the hinges free
        body = tc.resolved(tc.FINGER_TOOL, scene).body
        cfg = sim.sim.ik_config(body)
        assert (cfg.mode, cfg.max_iters, cfg.free_mask) == (1, 60, 0b0111111)
        np.testing.assert_allclose([cfg.tol_pos, cfg.tol_rot, cfg.rot_weight, cfg.damping, cfg.max_step], [1e-4, 1e-3, 0.1, 1e-6, 0.5], rtol=1e-6)
        lo, hi = ref.limits(body)
        np.testing.assert_array_equal(np.array(cfg.q_lo[:7]), lo.astype(np.float32)); np.testing.assert_array_equal(np.array(cfg.q_hi[:7]), hi.astype(np.float32))
        assert np.all(np.array(cfg.q_lo[7:]) == 0) and np.all(np.array(cfg.q_hi[7:]) == 0)
        with pytest.raises(TypeError):
            sim.sim.ik_config(body, no_such_setting=1)


def test_argument_and_state_errors():
    blobs = trc.blobs("banana")
    names = blobs["meta"]["body_names"]
    sim = TreeArraySim(blobs["f32"], 2, backend="emu")
    L, h = sim.sim.L, sim.sim.h
    err = lambda: L.so101_tree_last_error(h).decode()
    grip = tc.resolved("left/gripper")
    struct = lambda tool=grip: native.tool_spec(tool.spec())
    t = struct()
    ncol = 6
    # so101_tree_tool_chain / so101_tree_ik_default_config: which bodies can carry a tool
    buf = (C.c_int32 * 8)()
    cfg = native.TreeIkConfig()
    assert L.so101_tree_tool_chain(h, grip.body, buf, None, None) == 6 and L.so101_tree_tool_chain(h, grip.body, None, None, None) == 6
    assert L.so101_tree_tool_chain(None, grip.body, buf, None, None) == -1 and L.so101_tree_ik_default_config(None, grip.body, C.byref(cfg)) == -1
    assert L.so101_tree_ik_default_config(h, grip.body, None) == -1 and L.so101_tree_ik_default_config(h, grip.body, C.byref(cfg)) == 0
    for body, word in ((0, "1 .. nbody - 1"), (-1, "1 .. nbody - 1"), (len(names), "1 .. nbody - 1"), (names.index("table"), "no joint above"),
                       (names.index("object"), "free joint"), (names.index("container"), "free joint"), (names.index("left/base_link"), "no joint above")):
        assert L.so101_tree_tool_chain(h, body, buf, None, None) == -1 and word in err(), (body, err())
        assert L.so101_tree_ik_default_config(h, body, C.byref(native.TreeIkConfig())) == -1 and word in err(), (body, err())

    q = np.zeros((2, ncol), np.float32)
    pos, mat, jac = np.zeros((2, 3), np.float32), np.zeros((2, 9), np.float32), np.zeros((2, 6 * ncol), np.float32)
    idx = np.zeros(2, np.int32)
    P = lambda a: None if a is None else a.ctypes.data
    pose = lambda tool=t, q=q, idx=None, n=2, pos=pos, mat=mat, jac=jac, hh=h: L.so101_tree_tool_pose(hh, C.byref(tool) if tool is not None else None, P(q), P(idx), n, P(pos), P(mat), P(jac), None)
    assert pose() == 0 and pose(q=None) == 0 and pose(q=None, idx=idx) == 0 and pose(pos=None, mat=None) == 0
    assert pose(hh=None) == -1
    assert pose(tool=None) == -1 and "NULL tool" in err()
    for body, word in ((0, "1 .. nbody - 1"), (len(names), "1 .. nbody - 1"), (names.index("table"), "no joint above"), (names.index("object"), "free joint")):
        b = struct(); b.body = body
        assert pose(tool=b) == -1 and word in err(), (body, err())
    b = struct(); b.mat[0] = 1.001
    assert pose(tool=b) == -1 and "orthonormal" in err()
    b = struct(); b.mat[1] = 2e-4                     # a shear of 2e-4: |M^T M - I| = 2e-4
    assert pose(tool=b) == -1 and "orthonormal" in err()
    b = struct(); b.mat[1] = 5e-5                     # within 1e-4: accepted
    assert pose(tool=b) == 0
    b = struct(); b.pos[1] = float("inf")
    assert pose(tool=b) == -1 and "not finite" in err()
    assert pose(n=0) == -1 and pose(n=(1 << 26) + 1) == -1 and pose(q=None, n=3) == -1 and "exceeds" in err()
    assert pose(idx=idx) == -1 and "env_index" in err()
    assert pose(pos=None, mat=None, jac=None) == -1 and "no output" in err()

    tp, tm = np.zeros((2, 3), np.float32), np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (2, 1))
    qo, res, info = np.zeros((2, ncol), np.float32), np.zeros((2, 2), np.float32), np.zeros(2, np.int32)

    def ik(tool=t, c=cfg, tp=tp, tm=tm, qi=q, idx=None, n=2, qo=qo, res=res, info=info, hh=h):
        return L.so101_tree_tool_ik(hh, C.byref(tool) if tool is not None else None, C.byref(c) if c is not None else None, P(tp), P(tm), P(qi), P(idx), n,
                                    P(qo), P(res), P(info), None)

    def changed(**kw):
        c = native.TreeIkConfig.from_buffer_copy(cfg)
        for k, v in kw.items():
            if k in ("q_lo", "q_hi"):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c

    assert ik() == 0 and ik(res=None, info=None) == 0 and ik(qi=None) == 0 and ik(qi=None, idx=idx) == 0
    assert ik(hh=None) == -1 and ik(tool=None) == -1 and ik(c=None) == -1 and "NULL config" in err()
    b = struct(); b.body = names.index("table")
    assert ik(tool=b) == -1 and "no joint above" in err()
    assert ik(n=0) == -1 and ik(qi=None, n=3) == -1 and ik(idx=idx) == -1 and "env_index" in err()
    assert ik(tp=None) == -1 and ik(qo=None) == -1
    for bad in (dict(mode=-1), dict(mode=3), dict(max_iters=-1), dict(max_iters=1001), dict(tol_pos=0.0), dict(tol_rot=-1.0), dict(rot_weight=0.0),
                dict(max_step=0.0), dict(damping=-1e-9), dict(q_lo=(2, 4.0)), dict(tol_pos=float("nan"))):
        assert ik(c=changed(**bad)) == -1, bad
    assert ik(c=changed(q_lo=(7, 4.0))) == 0                      # beyond the chain's columns: ignored
    assert ik(c=changed(free_mask=1 << 6)) == -1 and "free_mask" in err() and ik(c=changed(free_mask=0x80000000)) == -1
    assert ik(c=changed(free_mask=0)) == 0 and ik(c=changed(free_mask=0b101)) == 0
    assert ik(c=changed(max_iters=0)) == 0 and ik(c=changed(max_iters=1000, damping=0.0)) == 0
    assert ik(tm=None) == -1 and "target_mat" in err()
    assert ik(c=changed(mode=2), tm=None) == -1 and ik(c=changed(mode=0), tm=None) == 0

    # nothing bound: explicit joint values work, the bound state is an error of call order
    un = native.TreeSim(blobs["f32"], 2, lib_path=sim.sim.L._name)
    assert pose(hh=un.h) == 0 and ik(hh=un.h) == 0
    assert pose(hh=un.h, q=None) == -4 and ik(hh=un.h, qi=None) == -4 and b"not bound" in L.so101_tree_last_error(un.h)
    un.close()


@pytest.mark.parametrize("scene", ["banana", "dining"])
def test_emulated_pose_and_jacobian_match_fp64(scene):
    ref = tc.reference(scene)
    states = np.stack([trc.STATES[k] for k in trc.STATE_NAMES] if scene == "banana" else [trc.DINING_STATE], axis=1)          # [nq, n]
    n = states.shape[1]
    sim = TreeArraySim(trc.blobs(scene)["f32"], n, backend="emu")
    sim.set_state(states)
    q32 = sim.get_state()[0]                          # the float32 qpos the kernels read
    for tool in tc.TOOLS:
        sp = tc.spec(tool, scene)
        qadr = ref.columns(sp[0])[1]
        pos, mat, jac = tc.tool_pose(sim, tool, n, scene=scene)
        pos2, mat2, jac2 = tc.tool_pose(sim, tool, n, q=q32[qadr].T, scene=scene)
        assert np.array_equal(pos, pos2) and np.array_equal(mat, mat2) and np.array_equal(jac, jac2)
        for e in range(n):
            p, M, J = ref.fk_qpos(q32[:, e], sp)
            err = (np.abs(pos[e] - p).max(), np.abs(mat[e] - M).max(), np.abs(jac[e] - J).max())
            print(f"emulated tool_pose {scene} {tc.resolved(tool).name} env {e}: |pos| {err[0]:.3e} m, |mat| {err[1]:.3e}, |jac| {err[2]:.3e}")
            assert err[0] <= POS_TOL and err[1] <= MAT_TOL and err[2] <= JAC_TOL
    if scene == "banana":
        # an env index outside the batch reads nothing: NaN outputs; the others are those of their envs
        pos, mat, jac = tc.tool_pose(sim, tc.FINGER_TOOL, 3)
        pos3, mat3, jac3 = tc.tool_pose(sim, tc.FINGER_TOOL, 4, env_index=[2, 3, -1, 0])
        assert np.array_equal(pos3[[0, 3]], pos[[2, 0]]) and np.array_equal(jac3[[0, 3]], jac[[2, 0]])
        assert np.isnan(pos3[1:3]).all() and np.isnan(mat3[1:3]).all() and np.isnan(jac3[1:3]).all()
    np.testing.assert_array_equal(sim.get_state()[0], states.astype(np.float32))              # no state changed


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_emulated_ik_reaches_the_first_cases(mode):
    ref = tc.reference()
    sim = TreeArraySim(trc.blobs("banana")["f32"], 1, backend="emu")
    n = 8
    for tool in ("left/gripper", tc.FINGER_TOOL):
        sp, cs = tc.spec(tool), tc.ik_cases(tool, 1)
        lo, hi = tc.limits(tool)
        q, res, info = tc.tool_ik(sim, tool, cs["pos"][:n], cs["mat"][:n], cs["q_init"][:n], mode=mode)
        print(f"emulated IK {tc.resolved(tool).name} mode {mode}: iterations {info.tolist()}")
        assert np.all(info >= 0) and np.all(info <= 60)
        assert np.all(q >= lo.astype(np.float32)) and np.all(q <= hi.astype(np.float32))
        if tool is tc.FINGER_TOOL:
            np.testing.assert_array_equal(q[:, 6], cs["q_init"][:n, 6].astype(np.float32))          # the finger's slide is held
        for i in range(n):
            rp, rr_ = ref.residual(q[i], sp, cs["pos"][i], cs["mat"][i], mode)
            assert rp <= 1e-4 + RES_POS and rr_ <= 1e-3 + RES_ROT, (i, rp, rr_)
            assert abs(res[i, 0] - rp) <= RES_POS and abs(res[i, 1] - rr_) <= RES_ROT
