"""fp64 reference of the depth / segmentation cameras of the general-tree engine (include/so101.h so101_tree_render).

tests/raycast_ref.RaycastRef with the forward kinematics of a general-tree blob (the ALOHA hand-over and Dining scenes) in place of
the SO100 chain's: every body has at most one joint - hinge, slide along the rotated axis, or free with a normalised quaternion - read
from `body_parent / body_jnttype / body_qposadr / body_pos / body_quat / arm_body / jnt_axis`.  A camera's body is a body id of the blob
(-1 or 0: the world).  The intersection code, the ambiguity rule (`image`), `assert_image`, DEPTH_RTOL and AMBIGUOUS_CAP are the parent's,
unchanged.
"""
from __future__ import annotations

import numpy as np

from tests import raycast_ref as rr

TJ_NONE, TJ_HINGE, TJ_FREE, TJ_SLIDE = 0, 1, 2, 3          # csrc/so101_tree.hpp


class TreeRaycastRef(rr.RaycastRef):
    def __init__(self, blob_f64: bytes):
        super().__init__(blob_f64)
        m = self.m
        self.nq = int(m["nq"][0])
        self.jtype, self.qadr = np.asarray(m["body_jnttype"]), np.asarray(m["body_qposadr"])
        self.jnt_of_body = {int(b): k for k, b in enumerate(m["arm_body"])}          # row of jnt_axis

    # ---- kinematics
    def body_frames(self, qpos):
        qpos = np.asarray(qpos, dtype=np.float64)
        nb = len(self.par)
        P, Q = np.zeros((nb, 3)), np.zeros((nb, 4))
        Q[0] = [1, 0, 0, 0]
        for b in range(1, nb):
            jt, a = int(self.jtype[b]), int(self.qadr[b])
            if jt == TJ_FREE:
                P[b] = qpos[a:a + 3]
                Q[b] = qpos[a + 3:a + 7] / np.linalg.norm(qpos[a + 3:a + 7])
                continue
            p = int(self.par[b])
            assert p < b, "bodies are numbered parents first"
            P[b] = P[p] + rr.q2m(Q[p]) @ self.bp[b]
            Q[b] = rr.qmul(Q[p], self.bq[b])
            if jt == TJ_HINGE:
                axis = self.axis[self.jnt_of_body[b]]
                Q[b] = rr.qmul(Q[b], np.r_[np.cos(0.5 * qpos[a]), np.sin(0.5 * qpos[a]) * axis])
            Q[b] /= np.linalg.norm(Q[b])
            if jt == TJ_SLIDE:
                P[b] = P[b] + rr.q2m(Q[b]) @ self.axis[self.jnt_of_body[b]] * qpos[a]
        return P, [rr.q2m(q) for q in Q]

    def camera_frame(self, qpos, cam):
        """cam = (body, pos, mat [3, 3] columns x y z, fovy_deg); body: -1 or 0 world, 1 .. nbody - 1 a body of the tree"""
        body, pos, mat, _ = cam
        pos, mat = np.asarray(pos, dtype=np.float64), np.asarray(mat, dtype=np.float64).reshape(3, 3)
        if body <= 0:
            return pos, mat
        P, R = self.body_frames(qpos)
        return P[body] + R[body] @ pos, R[body] @ mat
