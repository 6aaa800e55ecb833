"""fp64 reference of the contact interface (so101_contacts, include/so101.h): MuJoCo's frame completion, the reduction of a contact
list over pairs of geom groups, and the oracle's contact forces contact by contact.  numpy only; the kernels never run here."""
from __future__ import annotations

import numpy as np


def make_frame(normal):
    """mju_makeFrame as oracle/so101_oracle.cpp (make_frame) restates it: rows x = the unit normal, y = the y axis - or, when the normal
    is within 60 degrees of it (|x_y| >= 0.5), the z axis - made orthogonal to x and normalised, z = x cross y.  -> [3, 3], rows."""
    x = np.asarray(normal, dtype=np.float64)
    y = np.zeros(3)
    if -0.5 < x[1] < 0.5:
        y[1] = 1.0
    else:
        y[2] = 1.0
    y = y - (x @ y) * x
    y = y / np.linalg.norm(y)
    return np.stack([x, y, np.cross(x, y)])


def in_mask(mask, g) -> bool:
    """bit (g & 31) of word g >> 5 of a 4-word group mask"""
    return g >= 0 and bool((int(mask[g >> 5]) >> (g & 31)) & 1)


def pair_sign(a, b, g1, g2) -> int:
    """0: the contact (g1, g2) is not of the pair (a, b); -1: group a holds geom1 (tried first), +1: group a holds geom2.  The
    constraint force acts on geom2's body along the normal from geom1 to geom2, so the force ON group a is sign * R^T f[0:3]."""
    if in_mask(a, g1) and in_mask(b, g2):
        return -1
    if in_mask(a, g2) and in_mask(b, g1):
        return 1
    return 0


def both_orders(a, b, g1, g2) -> bool:
    return in_mask(a, g1) and in_mask(b, g2) and in_mask(a, g2) and in_mask(b, g1)


def reduce_pairs(pairs, geom, dist, frame=None, force=None):
    """The touch outputs of one env from its contact list, in fp64.  pairs: [(a mask, b mask)]; geom [k, 2], dist [k], frame [k, 9 or 3 x 3],
    force [k, 6] (the last two only for the force sums).  -> count [P] int, dist [P] (+inf without a contact), normal [P], force [P, 3],
    scale [P] = sum over the pair's contacts of |f_0| + |f_1| + |f_2| (what a rounding bound of the sums scales with)."""
    P = len(pairs)
    count, dmin = np.zeros(P, dtype=np.int64), np.full(P, np.inf)
    normal, net, scale = np.zeros(P), np.zeros((P, 3)), np.zeros(P)
    for p, (a, b) in enumerate(pairs):
        for k in range(len(geom)):
            s = pair_sign(a, b, int(geom[k][0]), int(geom[k][1]))
            if s == 0:
                continue
            count[p] += 1
            dmin[p] = min(dmin[p], float(dist[k]))
            if force is not None:
                R = np.asarray(frame[k], dtype=np.float64).reshape(3, 3)
                f = np.asarray(force[k], dtype=np.float64)
                normal[p] += f[0]
                net[p] += s * (R.T @ f[:3])
                scale[p] += np.abs(f[:3]).sum()
    return count, dmin, normal, net, scale


def oracle_contact_forces(o):
    """The forces of the oracle's last forward(), contact by contact: [ncon, 6], entries beyond a contact's dim zero.  The contact rows
    come last in efc_force, in contact order, dim rows each (make_constraints of the oracle); with elliptic cones they are the contact's
    force in its frame, which is what mj_contactForce returns."""
    cons = o.contacts()
    f = o.efc_force()
    rows = sum(c["dim"] for c in cons)
    assert rows <= len(f)
    tail = f[len(f) - rows:]
    out, at = np.zeros((len(cons), 6)), 0
    for k, c in enumerate(cons):
        out[k, :c["dim"]] = tail[at:at + c["dim"]]
        at += c["dim"]
    return out
