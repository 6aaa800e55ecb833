"""Cartesian tool control on the MI355X (so101_tool_pose / so101_tool_ik, include/so101.h) against the fp64 reference of tests/tool_ref.py.

Shapes: the kernels map one env to a lane, so the sizes that matter are n = 1, n = 65 (a second wavefront with a ragged tail) and n = 130
through env_index (a permutation with repeats of a 65-env batch).

Bounds.  Pose: position 2e-6 m, orientation entries 5e-6, Jacobian entries 5e-6 - an order of magnitude over the worst float32 emulation of
the same chain on 2000 states (1.6e-7 m, 6.4e-7, 7.9e-7); the margin covers the device's sincos and FMA contraction.  IK: FK_fp64(q_out)
lies within tol_pos + 2e-6 m and tol_rot + 1e-5 rad of the target (the margins are the pose bound; 1e-5 rad is what two orientation entries
5e-6 off can turn an angle by), and the reported residual is within those margins of the fp64 one."""
import numpy as np
import pytest

from tests import raycast_ref as rr, tool_cases as tc
from tests.simharness import ArraySim

pytestmark = pytest.mark.gpu
BACKEND = "gpu"
POS_TOL, MAT_TOL, JAC_TOL = 2e-6, 5e-6, 5e-6
RES_POS, RES_ROT = 2e-6, 1e-5
TOL_POS, TOL_ROT = 1e-4, 1e-3          # the default settings (so101_ik_default_config)

bits = lambda a: np.ascontiguousarray(a).view(np.int32)


def _rest(n):
    """[14, n] free-body part of a state: the props at rest"""
    return np.tile(rr.STATES["home"][6:, None], (1, n))


def _permutation_with_repeats(n_envs, n, seed):
    rs = np.random.RandomState(seed)
    idx = np.concatenate([rs.permutation(n_envs), rs.randint(0, n_envs, size=n - n_envs)]).astype(np.int32)
    assert len(set(idx.tolist())) == n_envs and len(idx) == n
    return idx


def test_pose_and_jacobian_against_fp64(blobs):
    ref = tc.reference()
    q = tc.random_q(11, 65)
    sim = ArraySim(blobs["f32"], 65, backend=BACKEND)
    sim.set_state(np.vstack([q.T, _rest(65)]))
    q32 = sim.get_state()[0][:6].T                      # the float32 joint angles the kernels read
    idx = _permutation_with_repeats(65, 130, 12)
    worst = np.zeros(3)
    for tool in (tc.pad_tool(), tc.JAW_TOOL, tc.IDENTITY_TOOL):
        want = [ref.fk(q32[e], tc.spec(tool)) for e in range(65)]
        for label, n, kw, rows in (("n=1", 1, dict(q=q32[:1]), range(1)), ("n=65", 65, dict(q=q32), range(65)),
                                   ("n=130 env_index", 130, dict(env_index=idx), idx)):
            pos, mat, jac = tc.tool_pose(sim, tool, n, **kw)
            err = np.array([max(np.abs(a[i] - want[e][k]).max() for i, e in enumerate(rows)) for k, a in enumerate((pos, mat, jac))])
            print(f"tool_pose {tool.name} {label}: worst |pos| {err[0]:.3e} m, |mat| {err[1]:.3e}, |jac| {err[2]:.3e}")
            worst = np.maximum(worst, err)
            assert err[0] <= POS_TOL and err[1] <= MAT_TOL and err[2] <= JAC_TOL, (tool.name, label, err)
            assert np.all(jac[:, :, tool.body + 1:] == 0)
            if "env_index" in kw:
                # q = NULL with env_index equals passing the gathered qpos explicitly, bit for bit
                p2, m2, j2 = tc.tool_pose(sim, tool, n, q=q32[idx])
                assert np.array_equal(bits(pos), bits(p2)) and np.array_equal(bits(mat), bits(m2)) and np.array_equal(bits(jac), bits(j2))
                # pose only, and an index outside the batch: NaN there, the same bits elsewhere
                bad = idx.copy(); bad[[3, 77]] = [65, -1]
                p3, m3, _ = tc.tool_pose(sim, tool, n, env_index=bad, jacobian=False)
                keep = np.ones(n, bool); keep[[3, 77]] = False
                assert np.isnan(p3[~keep]).all() and np.isnan(m3[~keep]).all()
                assert np.array_equal(bits(p3[keep]), bits(pos[keep])) and np.array_equal(bits(m3[keep]), bits(mat[keep]))
    print(f"tool_pose worst over all tools and shapes: |pos| {worst[0]:.3e} m, |mat| {worst[1]:.3e}, |jac| {worst[2]:.3e}")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_ik_reaches_the_target_in_fp64(blobs, mode):
    ref, tool, cs = tc.reference(), tc.pad_tool(), tc.ik_cases(1)
    n = 130
    sim = ArraySim(blobs["f32"], 65, backend=BACKEND)
    q, res, info = tc.tool_ik(sim, tool, cs["pos"][:n], cs["mat"][:n], cs["q_init"][:n], mode=mode)
    lo32, hi32 = ref.lo.astype(np.float32), ref.hi.astype(np.float32)
    worst = np.zeros(4)
    for i in range(n):
        rp, rr_ = ref.residual(q[i], tc.spec(tool), cs["pos"][i], cs["mat"][i], mode)
        worst = np.maximum(worst, [rp, rr_, abs(res[i, 0] - rp), abs(res[i, 1] - rr_)])
    print(f"tool_ik mode {mode}: iterations max {int(info.max())} mean {float(info.mean()):.2f}, not converged {int((info < 0).sum())}; fp64 residual "
          f"worst {worst[0]:.3e} m {worst[1]:.3e} rad; reported - fp64 worst {worst[2]:.3e} m {worst[3]:.3e} rad")
    assert np.all(info >= 0) and np.all(info <= 60), np.flatnonzero(info < 0)
    assert worst[0] <= TOL_POS + RES_POS and worst[1] <= TOL_ROT + RES_ROT
    assert worst[2] <= RES_POS and worst[3] <= RES_ROT
    assert np.all(q >= lo32) and np.all(q <= hi32)
    assert np.array_equal(bits(q[:, 5]), bits(cs["q_init"][:n, 5].astype(np.float32)))          # the jaw is beyond the tool's link
    # the other shapes give the same bits for the same entries: n = 1, n = 65, and n = 130 gathered from a bound 65-env state
    for m in (1, 65):
        q1, r1, i1 = tc.tool_ik(sim, tool, cs["pos"][:m], cs["mat"][:m], cs["q_init"][:m], mode=mode)
        assert np.array_equal(bits(q1), bits(q[:m])) and np.array_equal(bits(r1), bits(res[:m])) and np.array_equal(i1, info[:m])
    idx = _permutation_with_repeats(65, 130, 13)
    sim.set_state(np.vstack([cs["q_init"][:65].T, _rest(65)]))
    # entry i: the target of case i started from the joints of env idx[i]
    qe, re_, ie = tc.tool_ik(sim, tool, cs["pos"][:n], cs["mat"][:n], env_index=idx, mode=mode)
    qx, rx, ix = tc.tool_ik(sim, tool, cs["pos"][:n], cs["mat"][:n], cs["q_init"][idx], mode=mode)
    assert np.array_equal(bits(qe), bits(qx)) and np.array_equal(bits(re_), bits(rx)) and np.array_equal(ie, ix)
    same = np.flatnonzero(idx == np.arange(n) % 65)
    same = same[same < 65]
    assert np.array_equal(bits(qe[same]), bits(q[same]))
    bad = idx.copy(); bad[5] = 65
    qb, rb, ib = tc.tool_ik(sim, tool, cs["pos"][:n], cs["mat"][:n], env_index=bad, mode=mode)
    assert ib[5] == -1 and np.isnan(qb[5]).all() and np.isnan(rb[5]).all()
    keep = np.arange(n) != 5
    assert np.array_equal(bits(qb[keep]), bits(qe[keep])) and np.array_equal(ib[keep], ie[keep])


def test_ik_of_a_tool_on_an_inner_link(blobs):
    """a tool on link 2: three walked columns, three joints beyond it (tests/tool_cases.py check_inner_link)"""
    tc.check_inner_link(ArraySim(blobs["f32"], 1, backend=BACKEND), tc.N_INNER)


@pytest.mark.parametrize("mode", [1, 2])
def test_every_env_is_solved_independently(blobs, mode):
    """one wavefront of cases that start at their target, cases of seed 2 and one unreachable target: each entry's bits are those of solving it
    alone, although the wavefront loops until its slowest lane is done"""
    ref, tool, c1, c2 = tc.reference(), tc.pad_tool(), tc.ik_cases(1), tc.ik_cases(2)
    k = 21
    pos = np.concatenate([c1["pos"][:k], c2["pos"][:2 * k], c2["pos"][100:101] + [2.0, 0.0, 0.0]])
    mat = np.concatenate([c1["mat"][:k], c2["mat"][:2 * k], c2["mat"][100:101]])
    qi = np.concatenate([c1["q_target"][:k], c2["q_init"][:2 * k], c2["q_init"][100:101]])
    n = len(pos)
    assert n == 64
    sim = ArraySim(blobs["f32"], 1, backend=BACKEND)
    q, res, info = tc.tool_ik(sim, tool, pos, mat, qi, mode=mode)
    for i in range(n):
        q1, r1, i1 = tc.tool_ik(sim, tool, pos[i:i + 1], mat[i:i + 1], qi[i:i + 1], mode=mode)
        assert np.array_equal(bits(q1[0]), bits(q[i])) and np.array_equal(bits(r1[0]), bits(res[i])) and i1[0] == info[i], i
    print(f"independence mode {mode}: iterations {info.tolist()}")
    assert np.all(info[:k] == 0) and np.array_equal(bits(q[:k]), bits(qi[:k].astype(np.float32)))
    assert np.all(info[k:63] > 0)
    # the unreachable entry: not converged, after exactly max_iters iterations - its iterate follows the fp64 solve of the same length (the
    # damping e . e = 4 makes the steps small and smooth: float32 stays within 1e-3 rad of it), which has moved on since half that length
    assert info[63] == -1 and np.all(np.isfinite(q[63])) and np.all(q[63] >= ref.lo.astype(np.float32)) and np.all(q[63] <= ref.hi.astype(np.float32))
    want, winfo, _ = ref.ik(tc.spec(tool), pos[63], mat[63], qi[63], mode=mode)
    half, _, _ = ref.ik(tc.spec(tool), pos[63], mat[63], qi[63], mode=mode, max_iters=30)
    assert winfo == -1 and np.abs(want - half).max() > 1e-2
    assert np.abs(q[63] - want).max() <= 1e-3, np.abs(q[63] - want).max()
    r_end = ref.residual(q[63], tc.spec(tool), pos[63], mat[63], mode)
    r_start = ref.residual(np.clip(qi[63], ref.lo, ref.hi), tc.spec(tool), pos[63], mat[63], mode)
    w = 0.1
    assert np.hypot(r_end[0], w * r_end[1]) <= np.hypot(r_start[0], w * r_start[1])
    assert r_end[0] <= r_start[0]


def test_non_finite_targets_zero_iterations_and_tight_limits(blobs):
    ref, tool, cs = tc.reference(), tc.pad_tool(), tc.ik_cases(1)
    sim = ArraySim(blobs["f32"], 1, backend=BACKEND)
    lo32, hi32 = ref.lo.astype(np.float32), ref.hi.astype(np.float32)
    # non-finite targets among good ones; q_init partly outside the limits
    n = 6
    pos, mat, qi = cs["pos"][:n].copy(), cs["mat"][:n].copy(), cs["q_init"][:n].copy()
    pos[1, 2], pos[3, 0], mat[4, 1, 1] = np.nan, np.inf, -np.inf
    qi[1, 0], qi[3, 2] = 5.0, -1.0
    q, res, info = tc.tool_ik(sim, tool, pos, mat, qi, mode=1)
    clamped = np.clip(qi.astype(np.float32), lo32, hi32)
    for i in (1, 3, 4):
        assert info[i] == -1 and np.array_equal(bits(q[i]), bits(clamped[i])), i
    for i in (0, 2, 5):
        assert info[i] >= 0 and np.all(np.isfinite(q[i])) and np.all(np.isfinite(res[i]))
        rp, rr_ = ref.residual(q[i], tc.spec(tool), pos[i], mat[i], 1)
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
    qi[:, 1] = -1.25
    lo, hi = ref.lo.copy(), ref.hi.copy()
    lo[1] = hi[1] = -1.25
    q, res, info = tc.tool_ik(sim, tool, cs["pos"][:5], cs["mat"][:5], qi, mode=1, q_lo=lo, q_hi=hi)
    assert np.all(q[:, 1] == np.float32(-1.25)) and np.all(np.isfinite(q)) and np.all(q >= lo.astype(np.float32)) and np.all(q <= hi.astype(np.float32))


def test_tool_calls_change_no_state(blobs):
    names = ("home", "grasp", "tilted", "grasp")
    q0 = np.stack([rr.STATES[s] for s in names], axis=1)
    act = np.tile(np.array([0.3, -1.2, 1.3, 1.0, -0.5, 0.4], dtype=np.float32), (4, 1))
    cs = tc.ik_cases(1)

    def run(with_tool):
        sim = ArraySim(blobs["f32"], 4, backend=BACKEND, seed=3, last_step=500)
        sim.set_state(q0, np.zeros((18, 4)), np.zeros((6, 4)), np.zeros((18, 4)))
        sim.begin_episode()
        for _ in range(2):
            sim.step(act)
        if with_tool:
            tc.tool_pose(sim, tc.pad_tool(), 4)
            tc.tool_pose(sim, tc.JAW_TOOL, 3, env_index=[3, 1, 1])
            _, _, info = tc.tool_ik(sim, tc.pad_tool(), cs["pos"][:4], cs["mat"][:4], mode=2)
            assert len(info) == 4
        before = [sim._get(a) for a in (sim.qpos, sim.qvel, sim.ctrl, sim.warm)]
        sim.step(act)
        return before + [sim._get(a) for a in (sim.qpos, sim.qvel, sim.ctrl, sim.warm, sim.obs)]

    for a, b in zip(run(True), run(False)):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_batched_environment_cartesian_interface(blobs):
    """tool_pose / solve_ik / cartesian_action of a 4-env BatchedEnvironment.  The commanded ctrl: the step computes ctrl = action + offset
    in float32.  With zero offsets the bound ctrl IS the IK solution.  With non-zero offsets float32 has an action whose sum rounds to the
    solution q unless q - o falls into a higher binade than q (then the sums reach only every other float near q), and
    fl(q - o) is that action.  The test asserts the equality the interface promises - it holds for these inputs - and, so that a
    failure is readable, first that ctrl is action + offset and at most one unit in the last place of max(|q|, |q - o|) from q."""
    import torch
    from so101_sim_amd import task_suite
    ref, cs = tc.reference(), tc.ik_cases(1)
    env = task_suite.create_task_env("SO100HandOverBanana", time_limit=10.0, random_state=7, n_envs=4, settle_max_substeps=100, prefetch_resets=False)
    q0 = np.stack([rr.STATES[s] for s in ("home", "grasp", "tilted", "grasp")], axis=1)
    q0[:6] = cs["q_init"][:4].T
    env.qpos.copy_(torch.as_tensor(q0, dtype=torch.float32, device=env.device))
    env.qvel.zero_(); env.warm.zero_()
    env.begin_episode()
    q32 = env.qpos[:6].t().cpu().numpy()
    pad = tc.pad_tool()
    # tool_pose: shapes, devices, values
    pos, mat = env.tool_pose()
    assert pos.shape == (4, 3) and mat.shape == (4, 3, 3) and pos.dtype == torch.float32 and pos.device == env.qpos.device
    p2, m2, jac = env.tool_pose("fixed_jaw_pad", env_ids=[2, 0], jacobian=True)
    assert jac.shape == (2, 6, 6) and torch.equal(p2, pos[[2, 0]]) and torch.equal(m2, mat[[2, 0]])
    for e in range(4):
        p, M, J = ref.fk(q32[e], tc.spec(pad))
        assert np.abs(pos[e].cpu().numpy() - p).max() <= POS_TOL and np.abs(mat[e].cpu().numpy() - M).max() <= MAT_TOL
        if e in (2, 0):
            assert np.abs(jac[[2, 0].index(e)].cpu().numpy() - J).max() <= JAC_TOL
    p3, m3 = env.tool_pose(tc.JAW_TOOL, q=cs["q_target"][:3])
    for i in range(3):
        p, M, _ = ref.fk(cs["q_target"][i].astype(np.float32), tc.spec(tc.JAW_TOOL), jacobian=False)
        assert np.abs(p3[i].cpu().numpy() - p).max() <= POS_TOL and np.abs(m3[i].cpu().numpy() - M).max() <= MAT_TOL
    with pytest.raises(ValueError):
        env.tool_pose("no_such_tool")
    with pytest.raises(ValueError):
        env.tool_pose(env_ids=[4])
    with pytest.raises(ValueError):
        env.tool_pose(env_ids=[0], q=cs["q_target"][:1])
    # solve_ik round trip: from the current qpos to the targets of the cases, then the pose of the solution
    tp, tm = cs["pos"][:4], cs["mat"][:4]
    q, conv, res, iters = env.solve_ik(tp, tm)
    assert q.shape == (4, 6) and conv.dtype == torch.bool and res.shape == (4, 2) and iters.dtype == torch.int32
    assert bool(conv.all()) and bool((iters >= 0).all())
    pr, mr = env.tool_pose(q=q)
    assert float((pr - torch.tensor(tp, dtype=torch.float32, device=env.device)).norm(dim=1).max()) <= TOL_POS + RES_POS
    assert torch.equal(q[:, 5], env.qpos[5])
    q2, conv2, _, _ = env.solve_ik(tp[[3, 1]], mode=0, env_ids=[3, 1], max_iters=40)
    assert bool(conv2.all())
    q3, conv3, _, _ = env.solve_ik(tp, tm, mode=2, q_init=cs["q_init"][:4])
    assert bool(conv3.all())
    with pytest.raises(TypeError):
        env.solve_ik(tp, tm, no_such_setting=1)
    with pytest.raises(RuntimeError, match="max_iters"):
        env.solve_ik(tp, tm, max_iters=2000)
    # cartesian_action: zero offsets - the commanded ctrl is the solution with the jaw replaced, exactly
    assert all(float(x) == 0.0 for x in env.sim.cfg.action_offset)
    action = env.cartesian_action(tp, tm, jaw=0.5)
    assert action.shape == (4, 6)
    want = q.clone(); want[:, 5] = 0.5
    assert torch.equal(action, want)
    env.step_tensor(action)
    assert torch.equal(env.ctrl.t().contiguous(), want)
    # non-zero offsets
    off = [0.05, -0.03, 0.02, 0.01, -0.04, 0.015]
    env.sim.configure(action_offset=off)
    q4, _, _, _ = env.solve_ik(tp, tm)                # (from the state one control step on: the same solve cartesian_action runs)
    action = env.cartesian_action(tp, tm, jaw=0.5)
    want = q4.clone(); want[:, 5] = 0.5
    o = torch.tensor(off, dtype=torch.float32, device=env.device)
    env.step_tensor(action)
    ctrl = env.ctrl.t().contiguous()
    assert torch.equal(ctrl, action + o)
    ulp = torch.maximum(want.abs(), (want - o).abs()) * 2.0 ** -23
    print(f"cartesian_action with offsets: {int((ctrl == want).sum())} of {ctrl.numel()} commanded values equal the solution bit for bit, "
          f"worst difference {float((ctrl - want).abs().max()):.3e}")
    assert bool(((ctrl - want).abs() <= ulp).all())
    assert torch.equal(ctrl, want)
    env.close()
