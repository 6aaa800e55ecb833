"""fp64 reference of Cartesian tool control on the general-tree engine (include/so101.h so101_tree_tool_pose / so101_tree_tool_ik), numpy on
the f64 blob alone: the kinematics are tests/tree_raycast_ref.TreeRaycastRef.body_frames, body by body - nothing of the library's host-side
folding of jointless bodies - the Jacobian is MuJoCo's mj_jacSite (hinge (a x (p - o), a), slide (a, 0)), and the solve is the algorithm the
header writes down for so101_tool_ik over the chain's columns, with the free_mask."""
from __future__ import annotations

import numpy as np

from tests.tool_ref import dls_ik, errors, residual
from tests.tree_raycast_ref import TJ_FREE, TJ_HINGE, TJ_SLIDE, TreeRaycastRef


class TreeToolRef(TreeRaycastRef):
    def __init__(self, blob_f64: bytes):
        super().__init__(blob_f64)
        assert self.bp.dtype == np.float64, "the reference reads the f64 blob"
        self.dofadr = np.asarray(self.m["body_dofadr"])
        self.jrange = np.asarray(self.m["jnt_range"], dtype=np.float64).reshape(-1, 2)

    def chain(self, body):
        """bodies between the world and `body` that carry a hinge or slide joint, root first"""
        out, b = [], int(body)
        while b != 0:
            jt = int(self.jtype[b])
            assert jt != TJ_FREE, "a free joint in the chain"
            if jt in (TJ_HINGE, TJ_SLIDE):
                out.append(b)
            b = int(self.par[b])
        return out[::-1]

    def columns(self, body):
        """(dof, qposadr, jnt_type) of the chain's columns"""
        c = self.chain(body)
        return [int(self.dofadr[b]) for b in c], [int(self.qadr[b]) for b in c], [int(self.jtype[b]) for b in c]

    def limits(self, body):
        c = self.chain(body)
        r = np.array([self.jrange[self.jnt_of_body[b]] for b in c])
        return r[:, 0].copy(), r[:, 1].copy()

    def hinge_mask(self, body):
        return sum(1 << k for k, b in enumerate(self.chain(body)) if int(self.jtype[b]) == TJ_HINGE)

    def full_qpos(self, body, q, base=None):
        """a whole qpos with the chain's joints set to q (the other entries: `base`, or zeros with unit quaternions - they do not move the tool)"""
        if base is None:
            qpos = np.zeros(self.nq)
            for b in range(1, len(self.par)):
                if int(self.jtype[b]) == TJ_FREE:
                    qpos[int(self.qadr[b]) + 3] = 1.0
        else:
            qpos = np.array(base, dtype=np.float64)
        for b, v in zip(self.chain(body), np.asarray(q, dtype=np.float64)):
            qpos[int(self.qadr[b])] = v
        return qpos

    def fk_qpos(self, qpos, tool, jacobian=True):
        """tool = (body, pos, mat [3, 3]) at a whole qpos -> p [3], M [3, 3], J [6, ncol] (None without jacobian)"""
        body, pos, mat = tool
        P, R = self.body_frames(qpos)
        p = P[body] + R[body] @ np.asarray(pos, dtype=np.float64)
        M = R[body] @ np.asarray(mat, dtype=np.float64).reshape(3, 3)
        if not jacobian:
            return p, M, None
        c = self.chain(body)
        J = np.zeros((6, len(c)))
        for k, b in enumerate(c):
            a = R[b] @ self.axis[self.jnt_of_body[b]]
            if int(self.jtype[b]) == TJ_HINGE:
                J[:3, k], J[3:, k] = np.cross(a, p - P[b]), a
            else:
                J[:3, k] = a
        return p, M, J

    def fk(self, q, tool, jacobian=True):
        """the same at the chain's joint values q [ncol]"""
        return self.fk_qpos(self.full_qpos(tool[0], q), tool, jacobian)

    def errors(self, q, tool, target_pos, target_mat, mode):
        return errors(lambda x: self.fk(x, tool), q, target_pos, target_mat, mode)

    def residual(self, q, tool, target_pos, target_mat, mode):
        return residual(lambda x: self.fk(x, tool), q, target_pos, target_mat, mode)

    def ik(self, tool, target_pos, target_mat, q_init, lo=None, hi=None, free_mask=None, **cfg):
        """-> (q, info, (|e_p|, |e_r|)): dls_ik over the chain's columns; free_mask None = the hinge columns"""
        body = tool[0]
        dlo, dhi = self.limits(body)
        lo = dlo if lo is None else np.asarray(lo, dtype=np.float64)
        hi = dhi if hi is None else np.asarray(hi, dtype=np.float64)
        free_mask = self.hinge_mask(body) if free_mask is None else int(free_mask)
        free = np.array([(free_mask >> k) & 1 for k in range(len(lo))], dtype=bool)
        return dls_ik(lambda x: self.fk(x, tool), lo, hi, free, target_pos, target_mat, q_init, **cfg)
