"""TEST HARNESS ONLY: builds and loads list_rows_probe.hip - support_probe.hip plus the probe of k_narrow's list row pass - the way
tests/devprims/__init__.py builds support_probe.hip (same flags, same cache directory, keyed by a hash of every source read)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from tests import devprims

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "list_rows_probe.hip")
HL_ROW_MAX = 32          # so101_model.hpp: the longest list a row of 16 lanes holds, two entries per lane


def build(kind: str) -> str:
    if kind not in ("gpu", "emu"):
        raise ValueError(kind)
    return devprims.cached_build(SRC, kind, extra_inputs=[devprims.SRC])          # (the source includes support_probe.hip)


class Probes(devprims.Probes):
    """devprims.Probes over the library that also holds probe_list_rows"""

    def __init__(self, kind: str):
        self.kind = kind
        L = self.lib = C.CDLL(build(kind))
        vp, i = C.c_void_p, C.c_int
        L.probe_create.restype = vp
        L.probe_create.argtypes = [vp, i]
        L.probe_destroy.argtypes = [vp]
        L.probe_entry_count.argtypes = [vp]
        L.probe_tables.argtypes = [vp, vp, vp, vp]
        L.probe_pairs.argtypes = [vp, i, vp, vp, i, vp]
        L.probe_first_cell.argtypes = [vp, vp, i, vp]
        L.probe_list_rows.argtypes = [vp, i, vp, vp, i, vp]

    def list_rows(self, hull, chunk, g1, g2, rb):
        """the list row pass on (plane / box g1, `hull` posed by g2) pairs, `chunk` pairs per wavefront; returns what Hull.pairs() returns:
        settled (1 / 0, -1: the row pass does not serve the pair's list), valid mask, normal, distances, positions"""
        G, NC = devprims.GEOM_WORDS, devprims.NCPP
        pg = np.ascontiguousarray(np.concatenate([devprims._f32(g1, G), devprims._f32(g2, G)], axis=1))
        rb = devprims._f32(rb, 2)
        assert len(rb) == len(pg)
        self._check_finite(pg, rb)
        out = np.empty((len(pg), 5 + 4 * NC), np.float32)
        rc = self.lib.probe_list_rows(hull.h, chunk, pg.ctypes.data, rb.ctypes.data, len(pg), out.ctypes.data)
        assert rc == 0, rc
        return (out[:, 0].astype(int), out[:, 1].astype(np.uint32), out[:, 2:5], out[:, 5:5 + NC], out[:, 5 + NC:].reshape(-1, NC, 3))
