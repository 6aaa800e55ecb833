"""fp64 reference of Cartesian tool control (include/so101.h so101_tool_pose / so101_tool_ik), numpy on the f64 blob alone:
forward kinematics of the arm chain, the analytic Jacobian (MuJoCo's mj_jacSite: rows 0-2 jacp, rows 3-5 jacr), the rotation
vector, and the damped least-squares solve exactly as the header writes it down."""
from __future__ import annotations

import numpy as np

from so101_sim_amd.model import blob as blobfmt
from tests.raycast_ref import q2m, qmul

DEFAULTS = dict(mode=1, max_iters=60, tol_pos=1e-4, tol_rot=1e-3, rot_weight=0.1, damping=1e-6, max_step=0.5)


def rotvec_from(v, c, fallback):
    """axis * angle (angle in [0, pi]) from v = sin(angle) axis and c = cos(angle); at sin = 0: v for c > 0, pi * fallback otherwise"""
    s = np.linalg.norm(v)
    if s > 1e-12:
        return v * (np.arctan2(s, c) / s)
    return v.copy() if c > 0 else np.pi * np.asarray(fallback, dtype=np.float64)


def rotvec(R):
    """rotation vector of a rotation matrix, angle in [0, pi]; at pi: the column of R + I with the largest diagonal entry, normalised"""
    R = np.asarray(R, dtype=np.float64)
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    k = int(np.argmax(np.diag(R)))
    fb = (R + np.eye(3))[:, k]
    return rotvec_from(v, 0.5 * (np.trace(R) - 1.0), fb / max(np.linalg.norm(fb), 1e-300))


def zaxis_rotvec(z, zt):
    """rotation vector of the smallest rotation taking unit vector z to zt; at pi: z x e_k normalised, e_k where |z| is smallest"""
    ek = np.zeros(3)
    ek[int(np.argmin(np.abs(z)))] = 1.0
    fb = np.cross(z, ek)
    return rotvec_from(np.cross(z, zt), float(z @ zt), fb / np.linalg.norm(fb))


def errors(fk, q, target_pos, target_mat, mode):
    """fk: q -> (p, M, J).  -> (e_p, e_r, M, J) of the three modes"""
    p, M, J = fk(q)
    ep = np.asarray(target_pos, dtype=np.float64) - p
    if mode == 0:
        er = np.zeros(3)
    elif mode == 1:
        er = zaxis_rotvec(M[:, 2], np.asarray(target_mat, dtype=np.float64).reshape(3, 3)[:, 2])
    else:
        er = rotvec(np.asarray(target_mat, dtype=np.float64).reshape(3, 3) @ M.T)
    return ep, er, M, J


def residual(fk, q, target_pos, target_mat, mode):
    ep, er, _, _ = errors(fk, q, target_pos, target_mat, mode)
    return float(np.linalg.norm(ep)), float(np.linalg.norm(er))


def dls_ik(fk, lo, hi, free, target_pos, target_mat, q_init, **cfg):
    """-> (q, info, (|e_p|, |e_r|)): the algorithm of include/so101.h in fp64 over the columns of fk's Jacobian; free [ncol] bool: the columns
    solved for, the others are zero in Jw and keep clip(q_init)"""
    c = dict(DEFAULTS, **cfg)
    ncol = len(lo)
    mode, w = c["mode"], c["rot_weight"]
    q = np.clip(np.asarray(q_init, dtype=np.float64), lo, hi)
    finite = np.all(np.isfinite(target_pos)) and (mode == 0 or np.all(np.isfinite(target_mat)))
    it = 0
    while True:
        ep, er, M, J = errors(fk, q, target_pos, target_mat, mode)
        res = (float(np.linalg.norm(ep)), float(np.linalg.norm(er)))
        if not finite:
            return q, -1, res
        if res[0] <= c["tol_pos"] and res[1] <= c["tol_rot"]:
            return q, it, res
        if it == c["max_iters"]:
            return q, -1, res
        Jr = J[3:]
        if mode == 0:
            Jr = np.zeros((3, ncol))
        elif mode == 1:
            z = M[:, 2]
            Jr = (np.eye(3) - np.outer(z, z)) @ Jr
        Jw = np.vstack([J[:3], w * Jr])
        Jw[:, ~free] = 0.0
        e = np.r_[ep, w * er]
        A = Jw @ Jw.T + (e @ e + c["damping"]) * np.eye(6)
        L = np.linalg.cholesky(A)
        dq = Jw.T @ np.linalg.solve(L.T, np.linalg.solve(L, e))
        big = np.abs(dq).max()
        if big > c["max_step"]:
            dq = dq * (c["max_step"] / big)
        q = np.where(free, np.clip(q + dq, lo, hi), q)
        it += 1


class ToolRef:
    def __init__(self, blob_f64: bytes):
        m = blobfmt.unpack(blob_f64)
        assert m["body_pos"].dtype == np.float64, "the reference reads the f64 blob"
        self.bp, self.bq = m["body_pos"].reshape(-1, 3), m["body_quat"].reshape(-1, 4)
        self.par, self.arm = m["body_parent"], [int(b) for b in m["arm_body"]]
        self.axis = m["jnt_axis"].reshape(-1, 3)
        rng = m["jnt_range"].reshape(-1, 2)
        self.lo, self.hi = rng[:6, 0].copy(), rng[:6, 1].copy()
        # world pose of the arm's static base
        chain, b = [], int(self.par[self.arm[0]])
        while b != 0:
            chain.append(b)
            b = int(self.par[b])
        P, Q = np.zeros(3), np.array([1.0, 0, 0, 0])
        for b in reversed(chain):
            P, Q = P + q2m(Q) @ self.bp[b], qmul(Q, self.bq[b])
        self.base_p, self.base_q = P, Q / np.linalg.norm(Q)

    def links(self, q):
        """world origins o [6, 3], rotations R [6, 3, 3] and joint axes a [6, 3] of the arm links"""
        P, Q = self.base_p.copy(), self.base_q.copy()
        o, R, a = np.zeros((6, 3)), np.zeros((6, 3, 3)), np.zeros((6, 3))
        for k, b in enumerate(self.arm):
            P = P + q2m(Q) @ self.bp[b]
            Q = qmul(Q, self.bq[b])
            Q = qmul(Q, np.r_[np.cos(0.5 * q[k]), np.sin(0.5 * q[k]) * self.axis[k]])
            Q = Q / np.linalg.norm(Q)
            o[k], R[k], a[k] = P, q2m(Q), q2m(Q) @ self.axis[k]
        return o, R, a

    def fk(self, q, tool, jacobian=True):
        """tool = (body, pos, mat [3, 3] or [9] row-major) -> p [3], M [3, 3], J [6, 6] (None without jacobian)"""
        body, pos, mat = tool
        q = np.asarray(q, dtype=np.float64)
        o, R, a = self.links(q)
        p = o[body] + R[body] @ np.asarray(pos, dtype=np.float64)
        M = R[body] @ np.asarray(mat, dtype=np.float64).reshape(3, 3)
        if not jacobian:
            return p, M, None
        J = np.zeros((6, 6))
        for j in range(body + 1):
            J[:3, j], J[3:, j] = np.cross(a[j], p - o[j]), a[j]
        return p, M, J

    def errors(self, q, tool, target_pos, target_mat, mode):
        return errors(lambda x: self.fk(x, tool), q, target_pos, target_mat, mode)

    def residual(self, q, tool, target_pos, target_mat, mode):
        return residual(lambda x: self.fk(x, tool), q, target_pos, target_mat, mode)

    def ik(self, tool, target_pos, target_mat, q_init, lo=None, hi=None, **cfg):
        """-> (q, info, (|e_p|, |e_r|)): dls_ik over the six arm joints, all of them free"""
        lo = self.lo if lo is None else np.asarray(lo, dtype=np.float64)
        hi = self.hi if hi is None else np.asarray(hi, dtype=np.float64)
        return dls_ik(lambda x: self.fk(x, tool), lo, hi, np.ones(6, dtype=bool), target_pos, target_mat, q_init, **cfg)
