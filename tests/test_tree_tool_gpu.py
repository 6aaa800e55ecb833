"""Cartesian tool control of the general-tree engine on the MI355X (so101_tree_tool_pose / so101_tree_tool_ik, include/so101.h) against the
fp64 reference of tests/tree_tool_ref.py, on the HandOverBanana scene (32-dof build) and the Dining scene (64-dof build).

Shapes: the kernels map one entry to a lane, so the sizes that matter are n = 1, n = 65 (a second wavefront with a ragged tail) and n = 130
through env_index (a permutation with repeats of a 65-env batch).

Bounds.  Pose: position 3.4e-6 m, orientation entries 5.1e-6, Jacobian entries 4.9e-6 - one order of magnitude over the worst float32 numpy
evaluation of the same chain formulas on 2000 random states per tool (scripts/measure_tree_tool_bounds.py, on the CPU: 3.396e-7 m, 5.077e-7,
4.854e-7 over the four tools of tests/tree_tool_cases.py); the margin covers the device's sincos and FMA contraction.  IK: FK_fp64(q_out) lies
within tol_pos + 3.4e-6 m and tol_rot + 1.02e-5 rad of the target (the margins are the pose bound; 1.02e-5 rad is what two orientation entries
5.1e-6 off can turn an angle by), and the reported residual is within those margins of the fp64 one."""
import numpy as np
import pytest

from so101_sim_amd import native
from tests import tree_render_cases as trc, tree_tool_cases as tc
from tests.simharness import TreeArraySim

pytestmark = pytest.mark.gpu
BACKEND = "gpu"
POS_TOL, MAT_TOL, JAC_TOL = 3.4e-6, 5.1e-6, 4.9e-6
RES_POS, RES_ROT = POS_TOL, 2 * MAT_TOL
TOL_POS, TOL_ROT = 1e-4, 1e-3          # the default settings (so101_tree_ik_default_config)
ACTION = np.array([0.3, -0.6, 0.9, 0.2, -0.1, 0.3, 0.5, -0.3, -0.7, 1.0, -0.2, 0.1, -0.3, 0.8], dtype=np.float32)

bits = lambda a: np.ascontiguousarray(a).view(np.int32)


def _permutation_with_repeats(n_envs, n, seed):
    rs = np.random.RandomState(seed)
    idx = np.concatenate([rs.permutation(n_envs), rs.randint(0, n_envs, size=n - n_envs)]).astype(np.int32)
    assert len(set(idx.tolist())) == n_envs and len(idx) == n
    return idx


def _random_state(scene, n, seed):
    """[nq, n] qpos: the scene's props where the camera tests put them, every joint of both arms random within its range"""
    ref = tc.reference(scene)
    base = trc.STATES["home"] if scene == "banana" else trc.DINING_STATE
    qpos = np.tile(base[:, None], (1, n))
    for k, tool in enumerate(("left/left_finger", "left/right_finger", "right/left_finger", "right/right_finger")):
        body = tc.resolved(tool, scene).body
        lo, hi = ref.limits(body)
        qpos[ref.columns(body)[1]] = (lo + np.random.RandomState(seed + k).uniform(size=(n, len(lo))) * (hi - lo)).T
    return qpos


def _pose_against_fp64(scene, tool_list, shapes):
    ref = tc.reference(scene)
    sim = TreeArraySim(trc.blobs(scene)["f32"], 65, backend=BACKEND)
    sim.set_state(_random_state(scene, 65, 11))
    q32 = sim.get_state()[0]                          # [nq, 65]: the float32 qpos the kernels read
    idx = _permutation_with_repeats(65, 130, 12)
    worst = np.zeros(3)
    for tool in tool_list:
        sp = tc.spec(tool, scene)
        dof, qadr, _ = ref.columns(sp[0])
        assert tuple(sim.sim.tool_chain(sp[0])[:2]) == (dof, qadr)
        want = [ref.fk_qpos(q32[:, e], sp) for e in range(65)]
        qc = q32[qadr].T                              # [65, ncol]
        for label in shapes:
            n, kw, rows = {"n=1": (1, dict(q=qc[:1]), range(1)), "n=65": (65, dict(q=qc), range(65)), "n=130 env_index": (130, dict(env_index=idx), idx)}[label]
            pos, mat, jac = tc.tool_pose(sim, tool, n, scene=scene, **kw)
            assert jac.shape == (n, 6, len(dof))
            err = np.array([max(np.abs(a[i] - want[e][k]).max() for i, e in enumerate(rows)) for k, a in enumerate((pos, mat, jac))])
            print(f"tree tool_pose {scene} {tc.resolved(tool).name} {label}: worst |pos| {err[0]:.3e} m, |mat| {err[1]:.3e}, |jac| {err[2]:.3e}")
            worst = np.maximum(worst, err)
            assert err[0] <= POS_TOL and err[1] <= MAT_TOL and err[2] <= JAC_TOL, (tool, label, err)
            if "env_index" in kw:
                # q = NULL with env_index equals passing the gathered qpos explicitly, bit for bit
                p2, m2, j2 = tc.tool_pose(sim, tool, n, q=qc[idx], scene=scene)
                assert np.array_equal(bits(pos), bits(p2)) and np.array_equal(bits(mat), bits(m2)) and np.array_equal(bits(jac), bits(j2))
                # an index outside the batch: NaN there, the same bits elsewhere; once with the Jacobian, once pose only
                bad = idx.copy(); bad[[3, 77]] = [65, -1]
                keep = np.ones(n, bool); keep[[3, 77]] = False
                p3, m3, j3 = tc.tool_pose(sim, tool, n, env_index=bad, scene=scene)
                assert np.isnan(p3[~keep]).all() and np.isnan(m3[~keep]).all() and np.isnan(j3[~keep]).all()
                assert np.array_equal(bits(p3[keep]), bits(pos[keep])) and np.array_equal(bits(m3[keep]), bits(mat[keep])) and np.array_equal(bits(j3[keep]), bits(jac[keep]))
                p4, m4, _ = tc.tool_pose(sim, tool, n, env_index=bad, jacobian=False, scene=scene)
                assert np.array_equal(bits(p4[keep]), bits(pos[keep])) and np.isnan(p4[~keep]).all() and np.isnan(m4[~keep]).all()
    print(f"tree tool_pose {scene} worst over all tools and shapes: |pos| {worst[0]:.3e} m, |mat| {worst[1]:.3e}, |jac| {worst[2]:.3e}")


def test_pose_and_jacobian_against_fp64():
    _pose_against_fp64("banana", tc.TOOLS, ("n=1", "n=65", "n=130 env_index"))


def test_pose_and_jacobian_on_the_64_dof_build():
    _pose_against_fp64("dining", ("right/gripper", tc.FINGER_TOOL), ("n=65",))


@pytest.mark.parametrize("tool,mode", [(0, 0), (0, 1), (0, 2), (2, 1)])
def test_ik_reaches_the_target_in_fp64(tool, mode):
    tool = tc.TOOLS[tool]
    ref, sp, cs = tc.reference(), tc.spec(tool), tc.ik_cases(tool, 1)
    dof, qadr, types = ref.columns(sp[0])
    lo, hi = tc.limits(tool)
    n = 130
    sim = TreeArraySim(trc.blobs("banana")["f32"], 65, backend=BACKEND)
    q, res, info = tc.tool_ik(sim, tool, cs["pos"][:n], cs["mat"][:n], cs["q_init"][:n], mode=mode)
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    worst = np.zeros(4)
    for i in range(n):
        rp, rr_ = ref.residual(q[i], sp, cs["pos"][i], cs["mat"][i], mode)
        worst = np.maximum(worst, [rp, rr_, abs(res[i, 0] - rp), abs(res[i, 1] - rr_)])
    print(f"tree tool_ik {tc.resolved(tool).name} mode {mode}: iterations max {int(info.max())} mean {float(info.mean()):.2f}, not converged {int((info < 0).sum())}; "
          f"fp64 residual worst {worst[0]:.3e} m {worst[1]:.3e} rad; reported - fp64 worst {worst[2]:.3e} m {worst[3]:.3e} rad")
    assert np.all(info >= 0) and np.all(info <= 60), np.flatnonzero(info < 0)
    assert worst[0] <= TOL_POS + RES_POS and worst[1] <= TOL_ROT + RES_ROT
    assert worst[2] <= RES_POS and worst[3] <= RES_ROT
    assert np.all(q >= lo32) and np.all(q <= hi32)
    for k, t in enumerate(types):
        if t == native.TREE_JNT_SLIDE:               # held by default: the bits of q_init
            assert np.array_equal(bits(q[:, k]), bits(cs["q_init"][:n, k].astype(np.float32)))
    # the other shapes give the same bits for the same entries: n = 1, n = 65, and n = 130 gathered from a bound 65-env state
    for m in (1, 65):
        q1, r1, i1 = tc.tool_ik(sim, tool, cs["pos"][:m], cs["mat"][:m], cs["q_init"][:m], mode=mode)
        assert np.array_equal(bits(q1), bits(q[:m])) and np.array_equal(bits(r1), bits(res[:m])) and np.array_equal(i1, info[:m])
    idx = _permutation_with_repeats(65, 130, 13)
    qpos = _random_state("banana", 65, 14)
    qpos[qadr] = cs["q_init"][:65].T
    sim.set_state(qpos)
    # entry i: the target of case i started from the joints of env idx[i]
    qe, re_, ie = tc.tool_ik(sim, tool, cs["pos"][:n], cs["mat"][:n], env_index=idx, mode=mode)
    qx, rx, ix = tc.tool_ik(sim, tool, cs["pos"][:n], cs["mat"][:n], cs["q_init"][idx], mode=mode)
    assert np.array_equal(bits(qe), bits(qx)) and np.array_equal(bits(re_), bits(rx)) and np.array_equal(ie, ix)
    same = np.flatnonzero(idx[:65] == np.arange(65))
    assert np.array_equal(bits(qe[same]), bits(q[same]))
    bad = idx.copy(); bad[5] = 65
    qb, rb, ib = tc.tool_ik(sim, tool, cs["pos"][:n], cs["mat"][:n], env_index=bad, mode=mode)
    assert ib[5] == -1 and np.isnan(qb[5]).all() and np.isnan(rb[5]).all()
    keep = np.arange(n) != 5
    assert np.array_equal(bits(qb[keep]), bits(qe[keep])) and np.array_equal(ib[keep], ie[keep])


@pytest.mark.parametrize("mode", [1, 2])
def test_every_entry_is_solved_independently(mode):
    """one wavefront of cases that start at their target, cases of seed 2 and one unreachable target: each entry's bits are those of solving it
    alone, although the wavefront loops until its slowest lane is done"""
    tool = "left/gripper"
    ref, sp, c1, c2 = tc.reference(), tc.spec(tool), tc.ik_cases(tool, 1), tc.ik_cases(tool, 2)
    lo, hi = tc.limits(tool)
    k = 21
    pos = np.concatenate([c1["pos"][:k], c2["pos"][:2 * k], c2["pos"][100:101] + [2.0, 0.0, 0.0]])
    mat = np.concatenate([c1["mat"][:k], c2["mat"][:2 * k], c2["mat"][100:101]])
    qi = np.concatenate([c1["q_target"][:k], c2["q_init"][:2 * k], c2["q_init"][100:101]])
    n = len(pos)
    assert n == 64
    sim = TreeArraySim(trc.blobs("banana")["f32"], 1, backend=BACKEND)
    q, res, info = tc.tool_ik(sim, tool, pos, mat, qi, mode=mode)
    for i in range(n):
        q1, r1, i1 = tc.tool_ik(sim, tool, pos[i:i + 1], mat[i:i + 1], qi[i:i + 1], mode=mode)
        assert np.array_equal(bits(q1[0]), bits(q[i])) and np.array_equal(bits(r1[0]), bits(res[i])) and i1[0] == info[i], i
    print(f"tree independence mode {mode}: iterations {info.tolist()}")
    assert np.all(info[:k] == 0) and np.array_equal(bits(q[:k]), bits(qi[:k].astype(np.float32)))
    assert np.all(info[k:63] > 0)
    # the unreachable entry: not converged, finite, within the limits, and no further from the target than the start in the solve's own norm
    assert info[63] == -1 and np.all(np.isfinite(q[63])) and np.all(np.isfinite(res[63]))
    assert np.all(q[63] >= lo.astype(np.float32)) and np.all(q[63] <= hi.astype(np.float32))
    r_end = ref.residual(q[63], sp, pos[63], mat[63], mode)
    r_start = ref.residual(np.clip(qi[63], lo, hi), sp, pos[63], mat[63], mode)
    w = 0.1
    assert np.hypot(r_end[0], w * r_end[1]) <= np.hypot(r_start[0], w * r_start[1])


def test_non_finite_targets_zero_iterations_tight_limits_and_held_joints():
    tool = "left/gripper"
    ref, sp, cs = tc.reference(), tc.spec(tool), tc.ik_cases(tool, 1)
    lo, hi = tc.limits(tool)
    sim = TreeArraySim(trc.blobs("banana")["f32"], 1, backend=BACKEND)
    lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
    # non-finite targets among good ones; q_init partly outside the limits
    n = 6
    pos, mat, qi = cs["pos"][:n].copy(), cs["mat"][:n].copy(), cs["q_init"][:n].copy()
    pos[1, 2], pos[3, 0], mat[4, 1, 1] = np.nan, np.inf, -np.inf
    qi[1, 0], qi[3, 2] = 5.0, -4.0
    q, res, info = tc.tool_ik(sim, tool, pos, mat, qi, mode=1)
    clamped = np.clip(qi.astype(np.float32), lo32, hi32)
    assert clamped[1, 0] == hi32[0] and clamped[3, 2] == lo32[2]
    for i in (1, 3, 4):
        assert info[i] == -1 and np.array_equal(bits(q[i]), bits(clamped[i])), i
    for i in (0, 2, 5):
        assert info[i] >= 0 and np.all(np.isfinite(q[i])) and np.all(np.isfinite(res[i]))
        rp, rr_ = ref.residual(q[i], sp, pos[i], mat[i], 1)
        assert rp <= TOL_POS + RES_POS and rr_ <= TOL_ROT + RES_ROT
    q0, _, i0 = tc.tool_ik(sim, tool, pos, None, qi, mode=0)                  # mode 0 does not read the orientation
    assert i0[4] >= 0 and i0[1] == -1 and i0[3] == -1
    # max_iters = 0: clamp(q_init), info by the convergence test alone
    qi = np.concatenate([cs["q_target"][:3], cs["q_init"][:3]])
    qi[4, 0] = -9.0
    pos, mat = np.concatenate([cs["pos"][:3]] * 2), np.concatenate([cs["mat"][:3]] * 2)
    for mode in (0, 1, 2):
        q, res, info = tc.tool_ik(sim, tool, pos, mat, qi, mode=mode, max_iters=0)
        assert np.array_equal(bits(q), bits(np.clip(qi.astype(np.float32), lo32, hi32)))
        assert info.tolist() == [0, 0, 0, -1, -1, -1]
        assert np.all(res[:3, 0] <= RES_POS) and np.all(res[:3, 1] <= RES_ROT) and np.all(res[3:, 0] > TOL_POS)
    # q_lo = q_hi = q_init on one joint keeps that joint, whatever the target asks for
    qi = cs["q_init"][:5].copy()
    qi[:, 1] = -0.75
    l2, h2 = lo.copy(), hi.copy()
    l2[1] = h2[1] = -0.75
    assert lo[1] < -0.75 < hi[1]
    q, res, info = tc.tool_ik(sim, tool, cs["pos"][:5], cs["mat"][:5], qi, mode=1, q_lo=l2, q_hi=h2)
    assert np.all(q[:, 1] == np.float32(-0.75)) and np.all(np.isfinite(q)) and np.all(q >= l2.astype(np.float32)) and np.all(q <= h2.astype(np.float32))
    # a cleared free_mask bit on a hinge: that joint keeps clamp(q_init) bit for bit; five joints still reach a position (mode 0)
    n = 16
    qi = cs["q_init"][:n].copy()
    qi[:, 5] = cs["q_target"][:n, 5] + 0.25          # the wrist rotation is held off its target value; one row starts outside its limits
    qi[3, 5] = 9.0
    q, res, info = tc.tool_ik(sim, tool, cs["pos"][:n], None, qi, mode=0, free_mask=0b011111)
    print(f"tree tool_ik with the wrist rotation held, mode 0: iterations {info.tolist()}")
    assert np.array_equal(bits(q[:, 5]), bits(np.clip(qi[:, 5].astype(np.float32), lo32[5], hi32[5])))
    assert np.all(info >= 0) and np.all(info <= 60)
    for i in range(n):
        assert ref.residual(q[i], sp, cs["pos"][i], None, 0)[0] <= TOL_POS + RES_POS
    want = [ref.ik(sp, cs["pos"][i], None, qi[i], lo=lo, hi=hi, mode=0, free_mask=0b011111)[1] for i in range(n)]
    assert all(w >= 0 for w in want)                  # (a condition on the inputs: fp64 converges with that joint held)
    # all joints held: nothing moves
    q, _, info = tc.tool_ik(sim, tool, cs["pos"][:4], cs["mat"][:4], cs["q_init"][:4], mode=2, free_mask=0)
    assert np.array_equal(bits(q), bits(cs["q_init"][:4].astype(np.float32))) and np.all(info == -1)


def test_tool_calls_change_no_state():
    q0 = np.stack([trc.STATES[s] for s in ("home", "bent", "reach", "bent")], axis=1)
    act = np.stack([ACTION, -ACTION, ACTION, -ACTION])
    cs = tc.ik_cases("left/gripper", 1)

    def run(with_tool):
        sim = TreeArraySim(trc.blobs("banana")["f32"], 4, backend=BACKEND)
        sim.enable_env(n_substeps=2, settle_max_substeps=0)
        nv, nu = sim.sim.nv, sim.sim.nu
        sim.set_state(q0, np.zeros((nv, 4)), np.zeros((nu, 4)), np.zeros((nv, 4)))
        sim.begin_episode()
        for _ in range(2):
            sim.step(act)
        if with_tool:
            tc.tool_pose(sim, "left/gripper", 4)
            tc.tool_pose(sim, tc.FINGER_TOOL, 3, env_index=[3, 1, 1])
            _, _, info = tc.tool_ik(sim, "left/gripper", cs["pos"][:4], cs["mat"][:4], mode=2)
            assert len(info) == 4
        before = [sim._get(a) for a in (sim.qpos, sim.qvel, sim.ctrl, sim.warm)]
        sim.step(act)
        return before + [sim._get(a) for a in (sim.qpos, sim.qvel, sim.ctrl, sim.warm, sim.obs, sim.ring_pos, sim.ring_vel, sim.step_count)]

    for a, b in zip(run(True), run(False)):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_aloha_environment_cartesian_interface():
    """tool_pose / tool_chain / solve_ik / cartesian_action of a 4-env AlohaEnvironment.  The step neither clips nor converts arm entries of the
    action, so the ctrl commanded for a solved arm is the IK solution bit for bit."""
    import torch
    from so101_sim_amd import task_suite
    ref = tc.reference()
    env = task_suite.create_task_env("HandOverBanana", time_limit=10.0, random_state=7, n_envs=4, settle_max_substeps=100, prefetch_resets=False)
    env.reset()
    sp = tc.spec("left/gripper")
    q32 = env.qpos.t().cpu().numpy().astype(np.float64)          # [4, nq]
    # tool_chain and the default limits
    dof, qadr, types = env.tool_chain()
    assert (dof, qadr, types) == ref.columns(sp[0]) and dof == [0, 1, 2, 3, 4, 5]
    assert env.tool_chain("right/left_finger")[0] == [8, 9, 10, 11, 12, 13, 14] and env.tool_chain(tc.UPPER_TOOL)[0] == [0, 1]
    for tool in tc.TOOLS:
        lo, hi = env.ik_limits(tool)
        np.testing.assert_array_equal(lo, tc.limits(tool)[0]); np.testing.assert_array_equal(hi, tc.limits(tool)[1])
    assert env.ik_limits()[0][0] == -np.float32(np.pi / 2) and env.ik_limits("right/gripper")[1][0] == np.float32(np.pi / 2)
    # tool_pose: shapes, devices, values
    pos, mat = env.tool_pose()
    assert pos.shape == (4, 3) and mat.shape == (4, 3, 3) and pos.dtype == torch.float32 and pos.device == env.qpos.device
    p2, m2, jac = env.tool_pose("left/gripper", env_ids=[2, 0], jacobian=True)
    assert jac.shape == (2, 6, 6) and jac.dtype == torch.float32 and torch.equal(p2, pos[[2, 0]]) and torch.equal(m2, mat[[2, 0]])
    for e in range(4):
        p, M, J = ref.fk_qpos(q32[e], sp)
        assert np.abs(pos[e].cpu().numpy() - p).max() <= POS_TOL and np.abs(mat[e].cpu().numpy() - M).max() <= MAT_TOL
        if e in (2, 0):
            assert np.abs(jac[[2, 0].index(e)].cpu().numpy() - J).max() <= JAC_TOL
    fcs, fsp = tc.ik_cases(tc.FINGER_TOOL, 1), tc.spec(tc.FINGER_TOOL)
    p3, m3, j3 = env.tool_pose(tc.FINGER_TOOL, q=fcs["q_target"][:3], jacobian=True)
    assert j3.shape == (3, 6, 7)
    for i in range(3):
        p, M, J = ref.fk(fcs["q_target"][i].astype(np.float32), fsp)
        assert np.abs(p3[i].cpu().numpy() - p).max() <= POS_TOL and np.abs(m3[i].cpu().numpy() - M).max() <= MAT_TOL and np.abs(j3[i].cpu().numpy() - J).max() <= JAC_TOL
    with pytest.raises(ValueError):
        env.tool_pose("no_such_tool")
    with pytest.raises(TypeError):
        env.tool_pose(3)
    with pytest.raises(ValueError):
        env.tool_pose(env_ids=[4])
    with pytest.raises(ValueError):
        env.tool_pose(env_ids=[0], q=fcs["q_target"][:1, :6])
    with pytest.raises(ValueError):
        env.tool_pose(q=fcs["q_target"][:1])          # 7 values for a 6-column chain
    with pytest.raises(RuntimeError, match="free joint"):
        env.tool_pose(tc.tools.Tool("on_the_object", "object"))
    # solve_ik round trip: targets a few tenths of a radian from the current joints, then the pose of the solution
    lo, hi = tc.limits("left/gripper")
    u = np.random.RandomState(5).uniform(size=(4, 6))
    q_goal = np.clip(q32[:, qadr] + 0.25 * (2 * u - 1), lo, hi)
    tp, tm = env.tool_pose(q=q_goal)
    q, conv, res, iters = env.solve_ik(tp, tm)
    assert q.shape == (4, 6) and q.dtype == torch.float32 and conv.dtype == torch.bool and res.shape == (4, 2) and iters.dtype == torch.int32
    assert q.device == env.qpos.device and bool(conv.all()) and bool((iters >= 0).all())
    pr, mr = env.tool_pose(q=q)
    assert float((pr - tp).norm(dim=1).max()) <= TOL_POS + RES_POS
    q2, conv2, _, _ = env.solve_ik(tp[[3, 1]], mode=0, env_ids=[3, 1], max_iters=40)
    assert bool(conv2.all())
    q3, conv3, _, _ = env.solve_ik(tp, tm, mode=2, q_init=q32[:, qadr])
    assert bool(conv3.all())
    # a finger tool: 7 columns, the slide held at the current opening
    fq = env.tool_chain(tc.FINGER_TOOL)[1]
    ftp, ftm = env.tool_pose(tc.FINGER_TOOL, q=np.clip(q32[:, fq] + 0.2 * np.r_[2 * u[0] - 1, 0.0], *tc.limits(tc.FINGER_TOOL)))
    q4, conv4, _, _ = env.solve_ik(ftp, ftm, tool=tc.FINGER_TOOL)
    assert q4.shape == (4, 7) and bool(conv4.all()) and torch.equal(q4[:, 6], env.qpos[fq[6]])
    with pytest.raises(TypeError):
        env.solve_ik(tp, tm, no_such_setting=1)
    with pytest.raises(RuntimeError, match="max_iters"):
        env.solve_ik(tp, tm, max_iters=2000)
    with pytest.raises(RuntimeError, match="free_mask"):
        env.solve_ik(tp, tm, free_mask=1 << 6)
    with pytest.raises(ValueError):
        env.solve_ik(tp, tm, env_ids=[0, 1])
    # cartesian_action: the left arm solved, the right arm and the right gripper as commanded, the left gripper as given
    cmd = env.obs[:, 60:74].clone()
    g = torch.tensor([0.1, 0.5, 0.9, 1.2], dtype=torch.float32, device=env.device)
    action = env.cartesian_action(left=(tp, tm), right=None, gripper_left=g)
    assert action.shape == (4, 14) and action.dtype == torch.float32
    assert torch.equal(action[:, :6], q) and torch.equal(action[:, 6], g) and torch.equal(action[:, 7:], cmd[:, 7:])
    assert torch.equal(env.cartesian_action(), cmd)
    both = env.cartesian_action(left=(tp, None), right=(env.tool_pose("right/gripper")[0], None), gripper_right=0.3)
    assert torch.equal(both[:, 6], cmd[:, 6]) and bool((both[:, 13] == 0.3).all()) and torch.equal(both[:, 7:13], env.qpos[8:14].t())
    with pytest.raises(ValueError):
        env.cartesian_action(left=(tp[:2], tm[:2]))
    env.step_tensor(action)
    assert torch.equal(env.ctrl[:6].t().contiguous(), q)
    assert torch.equal(env.obs[:, 60:66], q)
    env.close()
