"""TEST HARNESS ONLY: builds and loads blocks_probe.hip - the cone blocks of both Newton solvers, the wave primitives and the small math - the way
tests/devprims/__init__.py builds support_probe.hip (same flags, same cache directory, keyed by a hash of every source read)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from tests import devprims

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "blocks_probe.hip")
SO100_CON_OUT, TREE_CON_OUT, QUAT_IN, QUAT_OUT, WAVE_CH = 39, 52, 32, 36, 4
WAVE_OPS = {n: k for k, n in enumerate(["max", "min_i", "sum", "sum_rows", "sum_row0", "ballot", "argmax", "argmax3", "row_argmax3", "row_argmax",
                                        "get", "bcast", "xor32"])}


def build(kind: str) -> str:
    if kind not in ("gpu", "emu"):
        raise ValueError(kind)
    return devprims.cached_build(SRC, kind)


def _a(x, dtype, shape=None):
    x = np.ascontiguousarray(np.asarray(x, dtype=dtype))
    return x if shape is None else x.reshape(shape)


class Probes:
    """The probe library of one build kind; every method takes and returns numpy arrays."""

    def __init__(self, kind: str):
        self.kind = kind
        L = self.lib = C.CDLL(build(kind))
        vp, i = C.c_void_p, C.c_int
        for name in ("probe_so100_contact", "probe_tree_contact"):
            getattr(L, name).argtypes = [i, vp, vp, vp, vp, vp, vp, vp]
        L.probe_so100_row.argtypes = [i, vp, vp, vp, vp]
        L.probe_tree_scalar.argtypes = [i, vp, vp, vp, vp, vp, vp]
        L.probe_sincos.argtypes = [i, vp, vp, vp]
        L.probe_quat.argtypes = [i, vp, vp]
        L.probe_impedance.argtypes = [i, vp, vp, vp]
        L.probe_rng.argtypes = [i, vp, vp, vp, vp, vp]
        L.probe_tri.argtypes = [i, vp]
        L.probe_wave.argtypes = [i, i, vp, vp, vp, vp]
        L.probe_mfma.argtypes = [i, i, vp, vp, vp]

    def _finite(self, *arrays):
        if self.kind == "gpu":
            for a in arrays:
                assert np.all(np.isfinite(a)), "non-finite inputs are for the emulated build only"

    def _contacts(self, fn, ow, dim, mu, fr, D, r, dr):
        n = len(dim)
        dim, mu, fr = _a(dim, np.int32), _a(mu, np.float32, (n,)), _a(fr, np.float32, (n, 5))
        D, r, dr = _a(D, np.float32, (n, 6)), _a(r, np.float32, (n, 6)), _a(dr, np.float32, (n, 6))
        self._finite(mu, fr, D, r, dr)
        out = np.empty((n, ow), np.float32)
        rc = fn(n, dim.ctypes.data, mu.ctypes.data, fr.ctypes.data, D.ctypes.data, r.ctypes.data, dr.ctypes.data, out.ctypes.data)
        assert rc == 0, rc
        return out

    def so100_contact(self, dim, mu, fr, D, r, dr):
        """contact_cost with and without the Hessian, contact_line: dict of cost, force (n, 6), Hc (n, 6, 6, from the packed lower triangle),
        zone, cost0, force0, zone0 (want_h off), d1, d2"""
        o = self._contacts(self.lib.probe_so100_contact, SO100_CON_OUT, dim, mu, fr, D, r, dr)
        H = np.zeros((len(o), 6, 6), np.float32)
        for k in range(6):
            for l in range(k + 1):
                H[:, k, l] = H[:, l, k] = o[:, 7 + k * (k + 1) // 2 + l]
        return dict(cost=o[:, 0], force=o[:, 1:7], Hc=H, zone=o[:, 28].astype(int), cost0=o[:, 29], force0=o[:, 30:36], zone0=o[:, 36].astype(int),
                    d1=o[:, 37], d2=o[:, 38])

    def tree_contact(self, dim, mu, fr, D, r, dr):
        """contact_block with and without the Hessian, the tree's contact_line: dict of cost, force, Hc (n, 6, 6 as stored), cost0, force0, d1, d2"""
        o = self._contacts(self.lib.probe_tree_contact, TREE_CON_OUT, dim, mu, fr, D, r, dr)
        return dict(cost=o[:, 0], force=o[:, 1:7], Hc=o[:, 7:43].reshape(-1, 6, 6), cost0=o[:, 43], force0=o[:, 44:50], d1=o[:, 50], d2=o[:, 51])

    def so100_row(self, R, floss, jar):
        R, floss, jar = _a(R, np.float32), _a(floss, np.float32), _a(jar, np.float32)
        self._finite(R, floss, jar)
        out = np.empty((len(R), 3), np.float32)
        rc = self.lib.probe_so100_row(len(R), R.ctypes.data, floss.ctypes.data, jar.ctypes.data, out.ctypes.data)
        assert rc == 0, rc
        return out

    def tree_scalar(self, type_, D, R, fl, r):
        t, D, R, fl, r = _a(type_, np.int32), _a(D, np.float32), _a(R, np.float32), _a(fl, np.float32), _a(r, np.float32)
        self._finite(D, R, fl, r)
        out = np.empty((len(t), 3), np.float32)
        rc = self.lib.probe_tree_scalar(len(t), t.ctypes.data, D.ctypes.data, R.ctypes.data, fl.ctypes.data, r.ctypes.data, out.ctypes.data)
        assert rc == 0, rc
        return out

    def sincos(self, x):
        x = _a(x, np.float32)
        self._finite(x)
        s, c = np.empty_like(x), np.empty_like(x)
        rc = self.lib.probe_sincos(len(x), x.ctypes.data, s.ctypes.data, c.ctypes.data)
        assert rc == 0, rc
        return s, c

    def quat(self, qa, qb, s6, R, m):
        """dict of quat2mat(qa), mulquat(qa, qb), normquat(qa), normalize3(qb[:3]) and its return value, rotsym(R, s6), mat2quat(m),
        rotvecquat(qb[1:], qa)"""
        n = len(qa)
        a = np.zeros((n, QUAT_IN), np.float32)
        a[:, 0:4], a[:, 4:8], a[:, 8:14], a[:, 14:23], a[:, 23:32] = qa, qb, s6, np.reshape(R, (n, 9)), np.reshape(m, (n, 9))
        self._finite(a)
        o = np.empty((n, QUAT_OUT), np.float32)
        rc = self.lib.probe_quat(n, a.ctypes.data, o.ctypes.data)
        assert rc == 0, rc
        return dict(quat2mat=o[:, 0:9].reshape(n, 3, 3), mulquat=o[:, 9:13], normquat=o[:, 13:17], normalize3=o[:, 17:20], norm3=o[:, 20],
                    rotsym=o[:, 21:27], mat2quat=o[:, 27:31], rotvecquat=o[:, 31:34])

    def impedance(self, solimp, pos):
        solimp, pos = _a(solimp, np.float32, (-1, 5)), _a(pos, np.float32)
        self._finite(solimp, pos)
        out = np.empty(len(pos), np.float32)
        rc = self.lib.probe_impedance(len(pos), solimp.ctypes.data, pos.ctypes.data, out.ctypes.data)
        assert rc == 0, rc
        return out

    def rng(self, seed, env, episode, draw):
        seed, env, ep, draw = _a(seed, np.uint64), _a(env, np.uint64), _a(episode, np.uint32), _a(draw, np.uint32)
        out = np.empty(len(seed), np.float32)
        rc = self.lib.probe_rng(len(seed), seed.ctypes.data, env.ctypes.data, ep.ctypes.data, draw.ctypes.data, out.ctypes.data)
        assert rc == 0, rc
        return out

    def tri(self, n):
        out = np.empty((n, n), np.int32)
        rc = self.lib.probe_tri(n, out.ctypes.data)
        assert rc == 0, rc
        return out

    def wave(self, op, f=None, i=None, ncase=None):
        """one 64-lane workgroup per case: f, i (ncase, <= WAVE_CH, 64) float32 / int32 channels (missing ones are zero); returns the float
        and int output channels, (ncase, WAVE_CH, 64) each"""
        ncase = ncase or len(f if f is not None else i)
        fin, iin = np.zeros((ncase, WAVE_CH, 64), np.float32), np.zeros((ncase, WAVE_CH, 64), np.int32)
        if f is not None:
            f = np.asarray(f, np.float32).reshape(ncase, -1, 64)
            fin[:, :f.shape[1]] = f
        if i is not None:
            i = np.asarray(i, np.int32).reshape(ncase, -1, 64)
            iin[:, :i.shape[1]] = i
        self._finite(fin)
        fo, io = np.empty_like(fin), np.empty_like(iin)
        rc = self.lib.probe_wave(WAVE_OPS[op], ncase, fin.ctypes.data, iin.ctypes.data, fo.ctypes.data, io.ctypes.data)
        assert rc == 0, rc
        return fo, io

    def mfma(self, a, b):
        """a, b (ncase, ncall, 64): returns the accumulators (ncase, 64, 16)"""
        a, b = _a(a, np.float32), _a(b, np.float32)
        assert a.shape == b.shape and a.shape[2] == 64
        self._finite(a, b)
        out = np.empty((a.shape[0], 64, 16), np.float32)
        rc = self.lib.probe_mfma(a.shape[0], a.shape[1], a.ctypes.data, b.ctypes.data, out.ctypes.data)
        assert rc == 0, rc
        return out
