"""Where the float32 bounds of the tree engine's tool-pose tests come from (tests/test_tree_tool_gpu.py, tests/test_tree_tool_emu.py).

    python scripts/measure_tree_tool_bounds.py [--states 2000]

A float32 numpy evaluation of the chain formulas of csrc/so101_tool_chain.hpp - the host's fold of the jointless bodies in double precision,
then per column xp += R pos, xq = xq * quat, hinge xq = xq * (cos q/2, axis sin q/2), normquat, slide xp += rot(axis, xq) q, and the Jacobian
columns - on random joint values within the default limits, for the four tools of tests/tree_tool_cases.py on the ALOHA blob, against the fp64
reference of tests/tree_tool_ref.py.  It runs on the CPU and does not touch the kernels under test.  Prints the worst differences in position
(metres), orientation entries and Jacobian entries; the tests' bounds are one order of magnitude over them.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from so101_sim_amd.model import blob as blobfmt          # noqa: E402
from tests import tree_render_cases as trc, tree_tool_cases as tc          # noqa: E402
from tests.tree_raycast_ref import TJ_HINGE, TJ_SLIDE          # noqa: E402

F = np.float32


def q2m(q):
    w, x, y, z = (q[..., i] for i in range(4))
    one, two = q.dtype.type(1), q.dtype.type(2)
    return np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                     two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                     two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], axis=-1).reshape(q.shape[:-1] + (3, 3))


def qmul(p, q):
    return np.stack([p[..., 0] * q[..., 0] - p[..., 1] * q[..., 1] - p[..., 2] * q[..., 2] - p[..., 3] * q[..., 3],
                     p[..., 0] * q[..., 1] + p[..., 1] * q[..., 0] + p[..., 2] * q[..., 3] - p[..., 3] * q[..., 2],
                     p[..., 0] * q[..., 2] - p[..., 1] * q[..., 3] + p[..., 2] * q[..., 0] + p[..., 3] * q[..., 1],
                     p[..., 0] * q[..., 3] + p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1] + p[..., 3] * q[..., 0]], axis=-1)


def fold(m, body, tpos, tmat):
    """the host's chain of a tool on `body` from the f32 blob: per column (pos, quat, axis, type), then the tool's folded (pos, mat), as float32"""
    bp, bq = m["body_pos"].reshape(-1, 3).astype(np.float64), m["body_quat"].reshape(-1, 4).astype(np.float64)
    par, jt = m["body_parent"], m["body_jnttype"]
    axis = {int(b): m["jnt_axis"].reshape(-1, 3)[k] for k, b in enumerate(m["arm_body"])}
    path, b = [], int(body)
    while b != 0:
        path.append(b)
        b = int(par[b])
    cols, P, Q = [], np.zeros(3), np.array([1.0, 0, 0, 0])
    for b in path[::-1]:
        P = P + q2m(Q) @ bp[b]
        Q = qmul(Q, bq[b] / np.linalg.norm(bq[b]))
        Q = Q / np.linalg.norm(Q)
        if int(jt[b]) in (TJ_HINGE, TJ_SLIDE):
            cols.append((P.astype(F), Q.astype(F), axis[b].astype(F), int(jt[b])))
            P, Q = np.zeros(3), np.array([1.0, 0, 0, 0])
    return cols, (P + q2m(Q) @ tpos).astype(F), (q2m(Q) @ tmat).astype(F)


def fk32(cols, tpos, tmat, q):
    """float32 throughout; q [n, ncol] -> p [n, 3], M [n, 3, 3], J [n, 6, ncol]"""
    n = len(q)
    xp, xq = np.zeros((n, 3), F), np.tile(np.array([1, 0, 0, 0], F), (n, 1))
    R = q2m(xq)
    o, a = [], []
    for k, (pos, quat, ax, jt) in enumerate(cols):
        xp = xp + np.einsum("nij,j->ni", R, pos)
        xq = qmul(xq, np.tile(quat, (n, 1)))
        if jt == TJ_HINGE:
            h = F(0.5) * q[:, k]
            jq = np.concatenate([np.cos(h)[:, None], np.sin(h)[:, None] * ax], axis=1).astype(F)
            xq = qmul(xq, jq)
        xq = xq / np.sqrt(np.sum(xq * xq, axis=1, dtype=F))[:, None]
        R = q2m(xq)
        if jt == TJ_SLIDE:
            xp = xp + np.einsum("nij,j->ni", R, ax) * q[:, k:k + 1]
        o.append(xp); a.append(np.einsum("nij,j->ni", R, ax))
    p = xp + np.einsum("nij,j->ni", R, tpos)
    M = np.einsum("nij,jk->nik", R, tmat)
    J = np.zeros((n, 6, len(cols)), F)
    for k, (_, _, _, jt) in enumerate(cols):
        if jt == TJ_HINGE:
            J[:, :3, k], J[:, 3:, k] = np.cross(a[k], p - o[k]), a[k]
        else:
            J[:, :3, k] = a[k]
    assert p.dtype == F and M.dtype == F
    return p, M, J


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=2000)
    args = ap.parse_args()
    ref = tc.reference()
    m = blobfmt.unpack(trc.blobs("banana")["f32"])
    worst = np.zeros(3)
    for t, tool in enumerate(tc.TOOLS):
        body, tpos, tmat = tc.spec(tool)
        cols, fp, fm = fold(m, body, tpos, tmat)
        q = tc.random_q(tool, 100 + t, args.states).astype(F)
        p, M, J = fk32(cols, fp, fm, q)
        err = np.zeros(3)
        for i in range(args.states):
            rp, rM, rJ = ref.fk(q[i].astype(np.float64), (body, tpos, tmat))
            err = np.maximum(err, [np.abs(p[i] - rp).max(), np.abs(M[i] - rM).max(), np.abs(J[i] - rJ).max()])
        print(f"{tc.resolved(tool).name:18s} {len(cols)} columns, {args.states} states: worst |pos| {err[0]:.3e} m, |mat| {err[1]:.3e}, |jac| {err[2]:.3e}")
        worst = np.maximum(worst, err)
    print(f"worst over the tools: |pos| {worst[0]:.3e} m, |mat| {worst[1]:.3e}, |jac| {worst[2]:.3e}")


if __name__ == "__main__":
    main()
