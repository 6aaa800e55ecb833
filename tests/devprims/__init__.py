"""TEST HARNESS ONLY: builds and loads the device probes of support_probe.hip (tests/test_support_queries.py).

kind="gpu": hipcc for gfx950 with exactly the product's flags (so101_sim_amd/build.py FLAGS: -ffp-contract=on is what makes the
            bit-identity of the support paths a property of the source rather than of the compiler's choices).
kind="emu": g++ against the lane-thread emulation of tests/hostemu, the way hostemu/emu_main.cpp builds the product.
Both are cached under tests/devprims/build/ by a hash of the compiler command and every source they read.
"""
from __future__ import annotations

import ctypes as C
import glob
import hashlib
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(_HERE))
SRC = os.path.join(_HERE, "support_probe.hip")
OUT = os.path.join(_HERE, "build")
EMU = os.path.join(ROOT, "tests", "hostemu")

# support paths of support_probe.hip: (name, path id, LDS slots)
PATHS = {"nocache": (0, 0), "hullcache": (1, 0), "lds256": (2, 256), "lds512": (2, 512), "lds0": (2, 0),
         "g16_256": (3, 256), "g16_512": (3, 512), "g16_0": (3, 0), "sub": (4, 0)}
# narrowphase paths of a flat face against a hull: the fused step's narrow_pair<NoCache>, k_narrow's fast path, k_narrow's row pass
PAIR_MODES = {"fused": 0, "fast": 1, "rows": 2}
HL_GRID, HL_CELLS, HL_MAX, SBT_GRID, NCPP = 8, 384, 128, 5, 5
GEOM_WORDS = 19


CSRC = os.path.join(ROOT, "so101_sim_amd", "csrc")


def cached_build(src: str, kind: str, defines=(), extra_inputs=(), program: bool = False) -> str:
    """The one probe build: compiles `src` unless tests/devprims/build/ already holds the result for this compiler command and these inputs.

    kind "gpu" / "emu": a shared library as described at the top of this file, its inputs `src` and every csrc/*.hpp (and, emulated, the two
    headers of tests/hostemu).  kind "host": plain host C++ with csrc/ and include/ on the include path, its input `src` alone; with `program` an
    executable with its own main instead of a shared library.  defines: "NAME=value" strings.  extra_inputs: further files the source reads.
    For "gpu", torch is imported first: PyTorch bundles its own HIP runtime, which must be the first one the process loads
    (so101_sim_amd/native.py load_library)."""
    if kind == "gpu":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        from so101_sim_amd import build as sbuild
        cmd = [sbuild.HIPCC, *sbuild.FLAGS, "-shared"]
    elif kind == "emu":
        cmd = [os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I" + EMU,
               "-include", os.path.join(EMU, "wave_emu.hpp"), "-Wno-unknown-pragmas", "-x", "c++"]
    elif kind == "host":
        cmd = [os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-I" + CSRC, "-I" + os.path.join(ROOT, "include")]
        cmd += [] if program else ["-fPIC", "-shared"]
    else:
        raise ValueError(kind)
    cmd = cmd[:1] + ["-D" + d for d in defines] + cmd[1:]
    inputs = [src]
    if kind != "host":
        inputs += sorted(glob.glob(os.path.join(CSRC, "*.hpp")))
    if kind == "emu":
        inputs += [os.path.join(EMU, "wave_emu.hpp"), os.path.join(EMU, "hip", "hip_runtime.h")]
    inputs += list(extra_inputs)
    h = hashlib.sha256(kind.encode())
    for a in cmd:
        h.update(os.path.basename(a).encode())
    for f in inputs:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    stem = os.path.splitext(os.path.basename(src))[0]
    out = os.path.join(OUT, f"{stem}_{kind}_{h.hexdigest()[:16]}" + ("" if program else ".so"))
    if not os.path.exists(out):
        os.makedirs(OUT, exist_ok=True)
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call(cmd + ["-o", tmp, src])
        os.replace(tmp, out)
    return out


def build(kind: str) -> str:
    if kind not in ("gpu", "emu"):
        raise ValueError(kind)
    return cached_build(SRC, kind)


def _f32(a, cols):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, cols))


class Probes:
    """The probe library of one build kind."""

    def __init__(self, kind: str):
        self.kind = kind
        L = self.lib = C.CDLL(build(kind))
        vp, i = C.c_void_p, C.c_int
        L.probe_create.restype = vp
        L.probe_create.argtypes = [vp, i]
        L.probe_destroy.argtypes = [vp]
        L.probe_entry_count.argtypes = [vp]
        L.probe_tables.argtypes = [vp, vp, vp, vp]
        L.probe_support.argtypes = [vp, i, i, i, vp, vp, i, vp]
        L.probe_hl_cell.argtypes = [vp, i, vp]
        L.probe_sbt_bound.argtypes = [vp, vp, i, C.c_float, vp]
        L.probe_pairs.argtypes = [vp, i, vp, vp, i, vp]
        L.probe_first_cell.argtypes = [vp, vp, i, vp]

    def _check_finite(self, *arrays):
        if self.kind == "gpu":
            for a in arrays:
                assert np.all(np.isfinite(a)), "non-finite inputs are for the emulated build only"

    def hull(self, V) -> "Hull":
        return Hull(self, V)

    def hl_cell(self, dl):
        dl = _f32(dl, 3)
        self._check_finite(dl)
        out = np.empty(len(dl), np.int32)
        rc = self.lib.probe_hl_cell(dl.ctypes.data, len(dl), out.ctypes.data)
        assert rc == 0, rc
        return out

    def first_cell(self, g1, g2):
        g1, g2 = _f32(g1, GEOM_WORDS), _f32(g2, GEOM_WORDS)
        assert len(g1) == len(g2)
        self._check_finite(g1, g2)
        out = np.empty(len(g1), np.int32)
        rc = self.lib.probe_first_cell(g1.ctypes.data, g2.ctypes.data, len(g1), out.ctypes.data)
        assert rc == 0, rc
        return out


class Hull:
    """One hull on the device, with the tables the product's builder makes for it."""

    def __init__(self, probes: Probes, V):
        self.P = probes
        self.V = _f32(V, 3)
        probes._check_finite(self.V)
        self.h = probes.lib.probe_create(self.V.ctypes.data, len(self.V))
        assert self.h, "probe_create failed"
        n = probes.lib.probe_entry_count(self.h)
        self.sbt = np.empty(6 * SBT_GRID * SBT_GRID, np.float32)
        self.off = np.empty(HL_CELLS + 1, np.uint32)
        ent = np.empty((max(n, 1), 4), np.float32)
        assert probes.lib.probe_tables(self.h, self.sbt.ctypes.data, self.off.ctypes.data, ent.ctypes.data) == 0
        self.entries = ent[:n]

    def close(self):
        if self.h:
            self.P.lib.probe_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def list_of(self, cell):
        """(indices, xyz) of a cell's support-vertex list"""
        e = self.entries[self.off[cell]:self.off[cell + 1]]
        return e[:, 3].view(np.int32), e[:, :3]

    def support(self, path: str, dirs, cells=None):
        return self._run(path, 0, _f32(dirs, 3), cells).reshape(-1, 3)

    def support_patch(self, path: str, frames, cells=None):
        """frames: (n, 9) = f | u | v"""
        return self._run(path, 1, _f32(frames, 9), cells).reshape(-1, NCPP, 3)

    def _run(self, path, patch, q, cells):
        pid, slots = PATHS[path]
        self.P._check_finite(q)
        c = None
        if pid == 4:
            c = np.ascontiguousarray(np.asarray(cells, dtype=np.int32))
            assert c.shape == (len(q),) and np.all((c >= 0) & (c < HL_CELLS))
        out = np.empty((len(q), 3 * NCPP if patch else 3), np.float32)
        rc = self.P.lib.probe_support(self.h, pid, slots, patch, q.ctypes.data, None if c is None else c.ctypes.data, len(q), out.ctypes.data)
        assert rc == 0, rc
        return out

    def sbt_bound(self, dl, pad=0.0):
        """pad: the value of the floats around the table on the device (a result that depends on it read outside the table)"""
        dl = _f32(dl, 3)
        self.P._check_finite(dl)
        out = np.empty(len(dl), np.float32)
        rc = self.P.lib.probe_sbt_bound(self.h, dl.ctypes.data, len(dl), C.c_float(pad), out.ctypes.data)
        assert rc == 0, rc
        return out

    def pairs(self, mode: str, g1, g2, rb):
        """narrowphase of (plane / box g1, this hull posed by g2) pairs on one path (PAIR_MODES); rb: (n, 2) bounding radii.
        Returns settled (1 / 0, -1: the path does not take the pair), valid mask, normal (n, 3), distances (n, NCPP), positions (n, NCPP, 3)."""
        pg = np.ascontiguousarray(np.concatenate([_f32(g1, GEOM_WORDS), _f32(g2, GEOM_WORDS)], axis=1))
        rb = _f32(rb, 2)
        assert len(rb) == len(pg)
        self.P._check_finite(pg, rb)
        out = np.empty((len(pg), 5 + 4 * NCPP), np.float32)
        rc = self.P.lib.probe_pairs(self.h, PAIR_MODES[mode], pg.ctypes.data, rb.ctypes.data, len(pg), out.ctypes.data)
        assert rc == 0, rc
        return (out[:, 0].astype(int), out[:, 1].astype(np.uint32), out[:, 2:5], out[:, 5:5 + NCPP],
                out[:, 5 + NCPP:].reshape(-1, NCPP, 3))
