"""Where the float32 bounds of tests/blocks_cases.py come from (tests/test_blocks_emu.py, tests/test_blocks_gpu.py).

    python scripts/measure_block_bounds.py

A float32 numpy restatement of the formulas - the elliptic cone block in the operation order of so101_newton.hpp and in that of so101_tree.hpp, the
line derivatives, the quaternion helpers and the solimp impedance of so101_math.hpp - evaluated on the committed cases of tests/blocks_cases.py
against their float64 references, with the tests' own error measures.  It runs on the CPU and does not touch the code under test.  Prints the
worst error per quantity; a test's bound is ten times that (an order of magnitude for fma contraction, operation order and the v_rcp / v_sqrt
based division and square root of the gfx950 build, none of which numpy can mirror).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import blocks_cases as bc          # noqa: E402

F = np.float32


def cone32(c, tree_order):
    """cost, force, Hc (n, 6, 6), d1, d2 in float32; zones decided in float32 as the kernels decide them"""
    dim, mu = c["dim"], c["mu"]
    n = len(dim)
    mask = np.arange(6)[None, :] < dim[:, None]
    r, dr, D = np.where(mask, c["r"], F(0)), np.where(mask, c["dr"], F(0)), np.where(mask, c["D"], F(0))
    fr = np.concatenate([np.zeros((n, 1), F), np.where(mask[:, 1:], c["fr"], F(0))], axis=1)
    U = r * fr
    U[:, 0] = r[:, 0] * mu
    T = np.sqrt(np.sum(U[:, 1:] * U[:, 1:], axis=1, dtype=F))
    N = U[:, 0]
    top = (dim == 0) | (N >= mu * T) | ((T <= 0) & (N >= 0))
    bot = ~top & ((mu * N + T <= 0) | ((T <= 0) & (N < 0)))
    mid = ~top & ~bot
    cost, force, H, d1, d2 = np.zeros(n, F), np.zeros((n, 6), F), np.zeros((n, 6, 6), F), np.zeros(n, F), np.zeros(n, F)
    cost[bot] = np.sum(F(0.5) * D * r * r, axis=1, dtype=F)[bot]
    force[bot] = (-D * r)[bot]
    H[bot] = (D[:, :, None] * np.eye(6, dtype=F))[bot]
    d1[bot], d2[bot] = np.sum(D * r * dr, axis=1, dtype=F)[bot], np.sum(D * dr * dr, axis=1, dtype=F)[bot]
    with np.errstate(all="ignore"):
        Dm = c["D"][:, 0] / np.maximum(mu * mu * (F(1) + mu * mu), F(bc.MINVAL))
        sN, iT = N - mu * T, F(1) / T
        f0 = -Dm * sN * mu
        if tree_order:
            fm = (-f0 / T)[:, None] * U * fr
            a = Dm * mu * mu
            Hm = (a[:, None, None] * fr[:, :, None] * fr[:, None, :] * U[:, :, None] * U[:, None, :] / (T * T)[:, None, None]
                  - (Dm * sN * mu)[:, None, None] * fr[:, :, None] * fr[:, None, :] * (np.eye(6, dtype=F)[None] / T[:, None, None] - U[:, :, None] * U[:, None, :] / (T * T * T)[:, None, None]))
            hk = -a[:, None] * U * fr / T[:, None]
        else:
            fm = (-f0 * iT)[:, None] * U * fr
            a, b = Dm * mu * mu, Dm * sN * mu
            w = U * fr * iT[:, None]
            Hm = a[:, None, None] * w[:, :, None] * w[:, None, :] - b[:, None, None] * ((fr * fr * iT[:, None])[:, :, None] * np.eye(6, dtype=F)[None] - w[:, :, None] * w[:, None, :] * iT[:, None, None])
            hk = -a[:, None] * w
        fm[:, 0] = f0
        Hm[:, 0, :], Hm[:, :, 0] = hk, hk
        Hm[:, 0, 0] = a
        du = dr * fr
        UdU, dUdU = np.sum(U[:, 1:] * du[:, 1:], axis=1, dtype=F), np.sum(du[:, 1:] * du[:, 1:], axis=1, dtype=F)
        dT = UdU * iT
        ddT, dS = (dUdU - dT * dT) * iT, dr[:, 0] * mu - mu * dT
    cost[mid] = (F(0.5) * Dm * sN * sN)[mid]
    force[mid], H[mid] = fm[mid], Hm[mid]
    d1[mid], d2[mid] = (Dm * sN * dS)[mid], (Dm * (dS * dS - sN * mu * ddT))[mid]
    for x in (cost, force, H, d1, d2):
        assert x.dtype == F
    zone = np.where(top, bc.ZONE_TOP, np.where(bot, bc.ZONE_BOTTOM, bc.ZONE_MIDDLE))
    return dict(cost=cost, force=force, Hc=H, d1=d1, d2=d2, zone=zone)


def q2m(q):
    w, x, y, z = (q[..., i] for i in range(4))
    one, two = F(1), F(2)
    return np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
                     two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
                     two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], axis=-1).reshape(q.shape[:-1] + (3, 3))


def m2q(m):
    m = m.reshape(-1, 9)
    br = bc.mat2quat_branch(m)
    q = np.zeros((len(m), 4), F)
    one = F(1)
    with np.errstate(all="ignore"):
        s = [np.sqrt(m[:, 0] + m[:, 4] + m[:, 8] + one) * F(2), np.sqrt(one + m[:, 0] - m[:, 4] - m[:, 8]) * F(2),
             np.sqrt(one + m[:, 4] - m[:, 0] - m[:, 8]) * F(2), np.sqrt(one + m[:, 8] - m[:, 0] - m[:, 4]) * F(2)]
        forms = [[F(0.25) * s[0], (m[:, 7] - m[:, 5]) / s[0], (m[:, 2] - m[:, 6]) / s[0], (m[:, 3] - m[:, 1]) / s[0]],
                 [(m[:, 7] - m[:, 5]) / s[1], F(0.25) * s[1], (m[:, 1] + m[:, 3]) / s[1], (m[:, 2] + m[:, 6]) / s[1]],
                 [(m[:, 2] - m[:, 6]) / s[2], (m[:, 1] + m[:, 3]) / s[2], F(0.25) * s[2], (m[:, 5] + m[:, 7]) / s[2]],
                 [(m[:, 3] - m[:, 1]) / s[3], (m[:, 2] + m[:, 6]) / s[3], (m[:, 5] + m[:, 7]) / s[3], F(0.25) * s[3]]]
    for b in range(4):
        q[br == b] = np.stack(forms[b], axis=1)[br == b]
    return q / np.sqrt(np.sum(q * q, axis=1, dtype=F))[:, None]


def quat32(c):
    qa, qb, s6, R = c["qa"], c["qb"], c["s6"], c["R"]
    S = np.stack([s6[:, 0], s6[:, 3], s6[:, 4], s6[:, 3], s6[:, 1], s6[:, 5], s6[:, 4], s6[:, 5], s6[:, 2]], axis=1).reshape(-1, 3, 3)
    RS = np.einsum("nij,njk->nik", np.einsum("nij,njk->nik", R, S), R.transpose(0, 2, 1))
    v = qb[:, :3]
    nv = np.sqrt(np.sum(v * v, axis=1, dtype=F))
    out = dict(quat2mat=q2m(qa), mulquat=bc.qmul64(qa, qb), normquat=qa / np.sqrt(np.sum(qa * qa, axis=1, dtype=F))[:, None],
               normalize3=v * (F(1) / nv)[:, None], norm3=nv,
               rotsym=np.stack([RS[:, 0, 0], RS[:, 1, 1], RS[:, 2, 2], RS[:, 0, 1], RS[:, 0, 2], RS[:, 1, 2]], axis=1),
               mat2quat=m2q(c["m"]), rotvecquat=np.einsum("nij,nj->ni", q2m(qa), qb[:, 1:]))
    for k, x in out.items():
        assert x.dtype == F, k
    return out


def impedance32(solimp, pos):
    lo, hi = F(bc.MINIMP), F(bc.MAXIMP)
    dmin, dmax, mid = np.clip(solimp[:, 0], lo, hi), np.clip(solimp[:, 1], lo, hi), np.clip(solimp[:, 3], lo, hi)
    width, p = np.maximum(solimp[:, 2], F(0)), np.maximum(solimp[:, 4], F(1))
    flat = (dmin == dmax) | (width <= F(bc.MINVAL))
    one = F(1)
    with np.errstate(all="ignore"):
        x = np.abs(pos) / np.where(flat, one, width)
        xc = np.clip(x, F(0), one)
        y2 = np.where(xc <= mid, xc * xc / mid, one - (one - xc) * (one - xc) / (one - mid))
        yp = np.where(xc <= mid, np.power(xc, p) / np.power(mid, p - one), one - np.power(one - xc, p) / np.power(one - mid, p - one))
        y = np.where(p == 1, xc, np.where(p == 2, y2, yp))
        out = np.where(flat, F(0.5) * (dmin + dmax), np.where(x >= 1, dmax, np.where(x <= 0, dmin, dmin + y * (dmax - dmin))))
    assert out.dtype == F
    return out


def main():
    print("cone blocks (tests/blocks_cases.py contact_cases), float32 restatement against float64 autograd:")
    c, ref = bc.contact_cases(False), bc.contact_reference(False)
    active = ref["zone"] != bc.ZONE_TOP
    table = {}
    for order in (False, True):
        got = cone32(c, order)
        assert np.array_equal(got["zone"], ref["zone"]), "a case lies too close to a zone boundary"
        e = bc.contact_errors(got, ref, active)
        for k, v in e.items():
            print(f"  {'so101_tree.hpp order' if order else 'so101_newton.hpp order'} {k:6s} worst {v.max():.3e}")
            table[k] = max(table.get(k, 0.0), float(v.max()))
    for k, name in bc.CON_BOUNDS.items():
        print(f"  {name:10s} measured {table[k]:.3e} -> bound {10 * table[k]:.1e} (tests: {getattr(bc, name):.1e})")
    print("quaternion helpers (quat_cases):")
    qc = bc.quat_cases()
    e = bc.quat_errors(quat32(qc), qc)
    for k, name in bc.QUAT_BOUNDS.items():
        print(f"  {name:10s} measured {e[k].max():.3e} -> bound {10 * e[k].max():.1e} (tests: {getattr(bc, name):.1e})")
    print("impedance (impedance_cases):")
    solimp, pos = bc.impedance_cases()
    err = np.abs(impedance32(solimp, pos) - bc.impedance_reference(solimp, pos))
    for p in (1.0, 2.0, 3.0):
        print(f"  power {p:g}: worst {err[solimp[:, 4] == p].max():.3e}")
    print(f"  {'IMPEDANCE':10s} measured {err.max():.3e} -> bound {10 * err.max():.1e} (tests: {bc.IMPEDANCE:.1e})")


if __name__ == "__main__":
    main()
