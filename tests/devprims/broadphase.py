"""TEST HARNESS ONLY: builds and loads broadphase_probe.hip - the product's two broadphases on body frames given directly - the way
tests/devprims/__init__.py builds support_probe.hip (same flags, same cache directory, keyed by a hash of every source read).  Three
builds per kind: engine 0 (SO100, so101_device.hpp), 32 and 64 (the two builds of so101_tree.hpp)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from tests import devprims

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "broadphase_probe.hip")
ENGINES = (0, 32, 64)
SBT_GRID = devprims.SBT_GRID
SBT_DIM = 6 * SBT_GRID * SBT_GRID


def build(kind: str, engine: int) -> str:
    if kind not in ("gpu", "emu") or engine not in ENGINES:
        raise ValueError((kind, engine))
    return devprims.cached_build(SRC, kind, defines=[f"BP_ENGINE={engine}"], extra_inputs=[os.path.join(devprims.ROOT, "include", "so101.h")])


class Probe:
    """One scene's geometry on one engine build.  `frames`: for engine 0 (geom_dyn [ngeom], geom_pos [ngeom, 3], geom_mat [ngeom, 3, 3]), the
    tree builds take theirs from the blob.  `sbt` False: SO101_NO_SBT is set while the model is built, as the product reads it at create."""

    def __init__(self, kind: str, engine: int, blob_f32: bytes, frames=None, sbt: bool = True):
        self.kind, self.engine = kind, engine
        L = self.lib = C.CDLL(build(kind, engine))
        vp, i = C.c_void_p, C.c_int
        L.probe_error.restype = C.c_char_p
        L.probe_create.restype = vp
        L.probe_create.argtypes = [C.c_char_p, C.c_size_t, vp, vp, vp]
        L.probe_destroy.argtypes = [vp]
        L.probe_dims.argtypes = [vp]
        L.probe_info.argtypes = [vp, vp]
        L.probe_tables.argtypes = [vp, vp, vp]
        L.probe_frames.argtypes = [vp, vp, vp, vp]
        L.probe_broadphase.argtypes = [vp, vp, vp, i, vp, vp, vp]
        dims = np.zeros(4, np.int32)
        L.probe_dims(dims.ctypes.data)
        self.nb, self.cap, self.ngeom_max = int(dims[0]), int(dims[1]), int(dims[2])
        assert int(dims[3]) == engine
        args = [None, None, None]
        if engine == 0:
            gd, gp, gm = frames
            keep = (np.ascontiguousarray(gd, dtype=np.int32), np.ascontiguousarray(gp, dtype=np.float32), np.ascontiguousarray(gm, dtype=np.float32))
            args = [a.ctypes.data for a in keep]
        old = os.environ.pop("SO101_NO_SBT", None)
        try:
            if not sbt:
                os.environ["SO101_NO_SBT"] = "1"
            self.h = L.probe_create(blob_f32, len(blob_f32), *args)
        finally:
            os.environ.pop("SO101_NO_SBT", None)
            if old is not None:
                os.environ["SO101_NO_SBT"] = old
        assert self.h, L.probe_error().decode()
        info = np.zeros(3, np.int32)
        assert L.probe_info(self.h, info.ctypes.data) == 0
        self.ngeom, self.npair, self.has_sbt = int(info[0]), int(info[1]), bool(info[2])
        assert self.has_sbt == sbt
        self.packed = np.zeros(max(self.npair, 1), np.uint32)
        self.sbt = np.zeros((self.ngeom, 6, SBT_GRID, SBT_GRID), np.float32)
        assert L.probe_tables(self.h, self.packed.ctypes.data, self.sbt.ctypes.data) == 0
        self.packed = self.packed[:self.npair]
        self.geom_dyn, self.geom_pos, self.geom_mat = np.zeros(self.ngeom, np.int32), np.zeros((self.ngeom, 3), np.float32), np.zeros((self.ngeom, 3, 3), np.float32)
        assert L.probe_frames(self.h, self.geom_dyn.ctypes.data, self.geom_pos.ctypes.data, self.geom_mat.ctypes.data) == 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.probe_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def run(self, xpos, xmat):
        """xpos [nq, nb, 3], xmat [nq, nb, 3, 3] -> ncand [nq], cand [nq, cap] (the whole candidate store, geom1 | geom2 << 16, 0xffffffff where the call wrote nothing), overflow [nq]"""
        xpos = np.ascontiguousarray(xpos, dtype=np.float32).reshape(-1, self.nb, 3)
        xmat = np.ascontiguousarray(xmat, dtype=np.float32).reshape(-1, self.nb, 9)
        nq = len(xpos)
        assert len(xmat) == nq
        if self.kind == "gpu":
            assert np.all(np.isfinite(xpos)) and np.all(np.isfinite(xmat)), "non-finite inputs are for the emulated build only"
        ncand, cand, over = np.full(nq, -7, np.int32), np.zeros((nq, self.cap), np.uint32), np.full(nq, -7, np.int32)
        rc = self.lib.probe_broadphase(self.h, xpos.ctypes.data, xmat.ctypes.data, nq, ncand.ctypes.data, cand.ctypes.data, over.ctypes.data)
        assert rc == 0, rc
        return ncand, cand, over
