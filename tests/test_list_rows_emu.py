"""CPU-only: the list row pass of k_narrow<false> (four list-backed flat-face pairs per wavefront, SO101_NARROW_LIST_ROWS) under the
lane-thread emulation of tests/hostemu - the launch chains with the pass on against the fused step, and the probe of tests/list_rows_cases.py
on a subset (the smallest bowl piece, the cube, and the 31- and 33-entry lists of the 308-vertex bowl piece).  tests/test_list_rows_gpu.py
runs everything on the MI355X."""
import pytest

from tests import list_rows_cases as lc
from tests import parity_cases as pc
from tests.devprims import list_rows
from tests.simharness import ArraySim


@pytest.fixture(scope="module")
def make_sim(blobs):
    def f(n, seed=0, **cfg):
        return ArraySim(blobs["f32"], n, backend="emu", seed=seed, **cfg)
    return f


@pytest.fixture(scope="module")
def emu():
    return list_rows.Probes("emu")


def test_list_row_pass_matches_fused(make_sim, golden, monkeypatch):
    monkeypatch.setenv("SO101_NARROW_LIST_ROWS", "1")
    pc.check_pipeline_identical(make_sim, golden, n=1, steps=1, settle=1, pipelines=(0, 1), first_state=9)


def test_list_rows_probe_emulated(emu, blobs):
    H = lc.hulls(blobs)
    seen, refused = {}, 0
    for name, lengths, tie in (("bowl:54", (1, 15, 16, 17, 32), False), ("cube:8", (1,), True), ("bowl:308", (31, 33), False)):
        hist, r = lc.check_hull(emu, H[name], name, lengths, tie=tie)
        refused += r
        for k, v in hist.items():
            seen[k] = seen.get(k, 0) + v
    assert all(seen.get(n, 0) >= 3 for n in lc.LENGTHS), seen      # (five poses settle per cell; the two tilted ones may land in a neighbour cell)
    assert refused >= 5, refused                                   # (the cell of 33 entries is not served)
