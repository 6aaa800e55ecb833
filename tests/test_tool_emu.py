"""Cartesian tool control without a GPU: self-checks of the fp64 reference (tests/tool_ref.py), solvability of the shared IK cases
(tests/tool_cases.py), the scene's tool table, and the library's argument checks, pose, Jacobian and IK through the emulated build of
the kernel source (tests/hostemu)."""
import ctypes as C

import numpy as np
import pytest

from so101_sim_amd import native, tools
from so101_sim_amd.model import blob as blobfmt
from tests import raycast_ref as rr, tool_cases as tc
from tests.simharness import ArraySim
from tests.tool_ref import ToolRef, rotvec, zaxis_rotvec

# float32 bounds of the pose test (tests/test_tool_gpu.py states where they come from)
POS_TOL, MAT_TOL, JAC_TOL = 2e-6, 5e-6, 5e-6


def test_so100_tool_table_comes_from_the_blob(blobs):
    m = blobfmt.unpack(blobs["f64"])
    t = tools.so100_tools(blobs["meta"], m)
    assert set(t) == {"fixed_jaw_pad"}
    pad = t["fixed_jaw_pad"]
    assert pad.body == 4 and pad.name == "fixed_jaw_pad"
    g = blobs["meta"]["geom_names"].index("fixed_jaw_pad_3")
    np.testing.assert_array_equal(pad.pos, m["geom_pos"].reshape(-1, 3)[g])
    np.testing.assert_allclose(pad.pos, (0.0126, -0.0768, 0.0), atol=1e-12)
    M = np.array(pad.mat)
    np.testing.assert_allclose(M.T @ M, np.eye(3), atol=1e-12)
    with pytest.raises(ValueError, match="unknown tool"):
        tools.resolve("gripper", t)
    q = tools.Tool.from_quat("t", 2, (0, 0, 0.1), (0.5, 0.5, 0.5, 0.5))
    np.testing.assert_allclose(np.array(q.mat) @ [1, 0, 0], [0, 1, 0], atol=1e-12)
    assert tools.Tool.from_xyaxes("t", 3, (0, 0, 0)).mat == ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))


def test_reference_pose_equals_the_camera_reference(blobs):
    ref, ray = ToolRef(blobs["f64"]), rr.RaycastRef(blobs["f64"])
    worst = 0.0
    for tool in (tc.pad_tool(), tc.JAW_TOOL, tc.IDENTITY_TOOL):
        for q in list(rr.STATES.values()) + [np.r_[x, rr.STATES["home"][6:]] for x in tc.random_q(3, 4)]:
            p, M, _ = ref.fk(q[:6], tc.spec(tool), jacobian=False)
            cp, cM = ray.camera_frame(q, (tool.body, tool.pos, np.array(tool.mat), 45.0))
            worst = max(worst, np.abs(p - cp).max(), np.abs(M - cM).max())
    print(f"tool reference vs camera reference: worst difference {worst:.3e}")
    assert worst <= 1e-12


def test_reference_jacobian_matches_central_differences(blobs):
    ref = ToolRef(blobs["f64"])
    h, worst = 1e-6, 0.0
    for tool in (tc.pad_tool(), tc.JAW_TOOL, tc.IDENTITY_TOOL):
        for q in tc.random_q(4, 6):
            _, M, J = ref.fk(q, tc.spec(tool))
            for j in range(6):
                d = np.zeros(6); d[j] = h
                pp, Mp, _ = ref.fk(q + d, tc.spec(tool), jacobian=False)
                pm, Mm, _ = ref.fk(q - d, tc.spec(tool), jacobian=False)
                W = (Mp - Mm) @ M.T / (2 * h)              # skew matrix of the angular velocity per unit joint rate
                num = np.r_[(pp - pm) / (2 * h), W[2, 1], W[0, 2], W[1, 0]]
                worst = max(worst, np.abs(num - J[:, j]).max())
            assert np.all(J[:, tool.body + 1:] == 0)
    print(f"analytic Jacobian vs central differences: worst difference {worst:.3e}")
    assert worst <= 1e-8


def test_reference_rotvec():
    rs = np.random.RandomState(5)
    for _ in range(20):
        ax = rs.normal(size=3); ax /= np.linalg.norm(ax)
        ang = rs.uniform(1e-3, np.pi - 1e-3)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
        np.testing.assert_allclose(rotvec(R), ang * ax, atol=1e-9)
        z = rs.normal(size=3); z /= np.linalg.norm(z)
        r = zaxis_rotvec(z, R @ z)
        assert abs(r @ z) < 1e-9 and np.linalg.norm(r) <= ang + 1e-9          # across z, and no longer than the rotation that made the target
        Kr = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) / np.linalg.norm(r)
        Rr = np.eye(3) + np.sin(np.linalg.norm(r)) * Kr + (1 - np.cos(np.linalg.norm(r))) * Kr @ Kr
        np.testing.assert_allclose(Rr @ z, R @ z, atol=1e-9)
    assert np.all(rotvec(np.eye(3)) == 0) and np.all(zaxis_rotvec(np.array([0, 0, 1.0]), np.array([0, 0, 1.0])) == 0)
    np.testing.assert_allclose(np.linalg.norm(rotvec(np.diag([1.0, -1.0, -1.0]))), np.pi)
    np.testing.assert_allclose(np.linalg.norm(zaxis_rotvec(np.array([0, 0, 1.0]), np.array([0, 0, -1.0]))), np.pi)


@pytest.mark.parametrize("seed", [1, 2])
def test_reference_ik_converges_on_every_shared_case(seed):
    """a condition on the inputs of the device tests: all 512 cases of the seed, all three modes, at most 10 iterations in fp64"""
    ref, tool, cs = tc.reference(), tc.spec(tc.pad_tool()), tc.ik_cases(seed)
    for mode in (0, 1, 2):
        worst = 0
        for i in range(tc.N_CASES):
            q, info, res = ref.ik(tool, cs["pos"][i], cs["mat"][i], cs["q_init"][i], mode=mode)
            assert 0 <= info <= 10, (seed, mode, i, info, res)
            assert np.all(q >= ref.lo) and np.all(q <= ref.hi)
            worst = max(worst, info)
        print(f"fp64 IK, seed {seed}, mode {mode}: 512/512 converged, worst {worst} iterations")


def test_reference_ik_converges_on_every_inner_link_case():
    """a condition on the inputs of the inner-link device tests: all 65 cases, position only, within the default 60 iterations in fp64"""
    ref, tool, cs = tc.reference(), tc.spec(tc.INNER_TOOL), tc.inner_cases()
    assert tool[0] == 2 and cs["pos"].shape == (65, 3) and cs["q_init"].shape == (65, 6)
    assert np.all(cs["q_init"] >= ref.lo) and np.all(cs["q_init"] <= ref.hi)
    infos = [ref.ik(tool, cs["pos"][i], None, cs["q_init"][i], mode=0)[1] for i in range(tc.N_INNER)]
    print(f"fp64 IK, inner-link cases: iterations {infos}")
    assert min(infos) >= 0 and max(infos) <= 60, infos


def _tool_struct(tool):
    return native.tool_spec(tool.spec())


def test_argument_and_state_errors(blobs):
    sim = ArraySim(blobs["f32"], 2, backend="emu")
    L, h = sim.sim.L, sim.sim.h
    err = lambda: L.so101_last_error(h).decode()
    t = _tool_struct(tc.pad_tool())
    cfg = native.IkConfig()
    assert L.so101_ik_default_config(h, C.byref(cfg)) == 0
    assert (cfg.mode, cfg.max_iters) == (1, 60)
    np.testing.assert_allclose([cfg.tol_pos, cfg.tol_rot, cfg.rot_weight, cfg.damping, cfg.max_step], [1e-4, 1e-3, 0.1, 1e-6, 0.5], rtol=1e-6)
    rng = blobfmt.unpack(blobs["f32"])["jnt_range"].reshape(-1, 2)
    np.testing.assert_array_equal(np.array(cfg.q_lo[:]), rng[:, 0]); np.testing.assert_array_equal(np.array(cfg.q_hi[:]), rng[:, 1])
    assert L.so101_ik_default_config(None, C.byref(cfg)) == -1 and L.so101_ik_default_config(h, None) == -1

    q = np.zeros((2, 6), np.float32)
    pos, mat, jac = np.zeros((2, 3), np.float32), np.zeros((2, 9), np.float32), np.zeros((2, 36), np.float32)
    idx = np.zeros(2, np.int32)
    P = lambda a: None if a is None else a.ctypes.data
    pose = lambda tool=t, q=q, idx=None, n=2, pos=pos, mat=mat, jac=jac, hh=h: L.so101_tool_pose(hh, C.byref(tool) if tool is not None else None, P(q), P(idx), n, P(pos), P(mat), P(jac), None)
    assert pose() == 0 and pose(q=None) == 0 and pose(q=None, idx=idx) == 0 and pose(pos=None, mat=None) == 0
    assert pose(hh=None) == -1
    assert pose(tool=None) == -1 and "NULL tool" in err()
    for body in (-1, 6):
        b = _tool_struct(tc.pad_tool()); b.body = body
        assert pose(tool=b) == -1 and "body" in err()
    b = _tool_struct(tc.pad_tool()); b.mat[0] = 1.001
    assert pose(tool=b) == -1 and "orthonormal" in err()
    b = _tool_struct(tc.pad_tool()); b.mat[1] = 2e-4                     # a shear of 2e-4: |M^T M - I| = 2e-4
    assert pose(tool=b) == -1 and "orthonormal" in err()
    b = _tool_struct(tc.pad_tool()); b.mat[1] = 5e-5                     # within 1e-4: accepted
    assert pose(tool=b) == 0
    assert pose(n=0) == -1 and pose(n=(1 << 26) + 1) == -1 and pose(q=None, n=3) == -1 and "exceeds" in err()
    assert pose(idx=idx) == -1 and "env_index" in err()
    assert pose(pos=None, mat=None, jac=None) == -1 and "no output" in err()

    tp, tm = np.zeros((2, 3), np.float32), np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (2, 1))
    qo, res, info = np.zeros((2, 6), np.float32), np.zeros((2, 2), np.float32), np.zeros(2, np.int32)

    def ik(tool=t, c=cfg, tp=tp, tm=tm, qi=q, idx=None, n=2, qo=qo, res=res, info=info, hh=h):
        return L.so101_tool_ik(hh, C.byref(tool) if tool is not None else None, C.byref(c) if c is not None else None, P(tp), P(tm), P(qi), P(idx), n,
                               P(qo), P(res), P(info), None)

    def changed(**kw):
        c = native.IkConfig.from_buffer_copy(cfg)
        for k, v in kw.items():
            if k in ("q_lo", "q_hi"):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c

    assert ik() == 0 and ik(res=None, info=None) == 0 and ik(qi=None) == 0 and ik(qi=None, idx=idx) == 0
    assert ik(hh=None) == -1 and ik(tool=None) == -1 and ik(c=None) == -1 and "NULL config" in err()
    b = _tool_struct(tc.pad_tool()); b.body = 6
    assert ik(tool=b) == -1
    assert ik(n=0) == -1 and ik(qi=None, n=3) == -1 and ik(idx=idx) == -1 and "env_index" in err()
    assert ik(tp=None) == -1 and ik(qo=None) == -1
    for bad in (dict(mode=-1), dict(mode=3), dict(max_iters=-1), dict(max_iters=1001), dict(tol_pos=0.0), dict(tol_rot=-1.0), dict(rot_weight=0.0),
                dict(max_step=0.0), dict(damping=-1e-9), dict(q_lo=(2, 4.0)), dict(tol_pos=float("nan"))):
        assert ik(c=changed(**bad)) == -1, bad
    assert ik(c=changed(max_iters=0)) == 0 and ik(c=changed(max_iters=1000, damping=0.0)) == 0
    assert ik(tm=None) == -1 and "target_mat" in err()
    assert ik(c=changed(mode=2), tm=None) == -1 and ik(c=changed(mode=0), tm=None) == 0

    # nothing bound: explicit joint angles work, the bound state is an error of call order
    un = native.Sim(blobs["f32"], 2, lib_path=sim.sim.L._name)
    assert pose(hh=un.h) == 0 and ik(hh=un.h) == 0
    assert pose(hh=un.h, q=None) == -4 and ik(hh=un.h, qi=None) == -4 and b"not bound" in L.so101_last_error(un.h)
    un.close()


def test_emulated_pose_and_jacobian_match_fp64(blobs):
    ref = tc.reference()
    states = np.stack([rr.STATES[k] for k in ("home", "grasp", "tilted")], axis=1)          # [20, 3]
    sim = ArraySim(blobs["f32"], 3, backend="emu")
    sim.set_state(states)
    for tool in (tc.pad_tool(), tc.JAW_TOOL):
        pos, mat, jac = tc.tool_pose(sim, tool, 3)
        pos2, mat2, jac2 = tc.tool_pose(sim, tool, 3, q=states[:6].T)
        assert np.array_equal(pos, pos2) and np.array_equal(mat, mat2) and np.array_equal(jac, jac2)
        for e in range(3):
            p, M, J = ref.fk(states[:6, e], tc.spec(tool))
            assert np.abs(pos[e] - p).max() <= POS_TOL and np.abs(mat[e] - M).max() <= MAT_TOL and np.abs(jac[e] - J).max() <= JAC_TOL
        assert np.all(jac[:, :, tool.body + 1:] == 0)
    # an env index outside the batch reads nothing: NaN outputs; the others are those of their envs
    pos3, mat3, jac3 = tc.tool_pose(sim, tc.JAW_TOOL, 4, env_index=[2, 3, -1, 0])
    assert np.array_equal(pos3[[0, 3]], pos[[2, 0]]) and np.array_equal(jac3[[0, 3]], jac[[2, 0]])
    assert np.isnan(pos3[1:3]).all() and np.isnan(mat3[1:3]).all() and np.isnan(jac3[1:3]).all()
    np.testing.assert_array_equal(sim.get_state()[0], states.astype(np.float32))              # no state changed


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_emulated_ik_reaches_the_first_cases(blobs, mode):
    ref, tool, cs = tc.reference(), tc.pad_tool(), tc.ik_cases(1)
    sim = ArraySim(blobs["f32"], 1, backend="emu")
    n = 8
    q, res, info = tc.tool_ik(sim, tool, cs["pos"][:n], cs["mat"][:n], cs["q_init"][:n], mode=mode)
    print(f"emulated IK mode {mode}: iterations {info.tolist()}")
    assert np.all(info >= 0) and np.all(info <= 60)
    assert np.all(q >= ref.lo.astype(np.float32)) and np.all(q <= ref.hi.astype(np.float32))
    np.testing.assert_array_equal(q[:, 5], cs["q_init"][:n, 5].astype(np.float32))
    for i in range(n):
        rp, rr_ = ref.residual(q[i], tc.spec(tool), cs["pos"][i], cs["mat"][i], mode)
        assert rp <= 1e-4 + 2e-6 and rr_ <= 1e-3 + 1e-5, (i, rp, rr_)
        assert abs(res[i, 0] - rp) <= 2e-6 and abs(res[i, 1] - rr_) <= 1e-5


def test_emulated_ik_of_a_tool_on_an_inner_link(blobs):
    tc.check_inner_link(ArraySim(blobs["f32"], 1, backend="emu"), 8)
