"""The two broadphases against fp64 on the MI355X (tests/devprims/broadphase_probe.hip built with the product's flags): the cases and checks of
tests/broadphase_cases.py, the reference of tests/broadphase_ref.py.  SO100 and ALOHA run the full families (a few hundred queries each),
Dining one case per cell and its four real states."""
import numpy as np
import pytest

from tests import broadphase_cases as bc

pytestmark = pytest.mark.gpu

KIND = "gpu"
SCENES = ("so100_banana", "so100_pen", "aloha", "dining")
T_PER_CELL, S_PER_CELL = 6, 25
S_CELL = ("type", "delta", "kind")
TREE_PLANES = ("so100_banana@32", "so100_banana@64")         # the SO100 scene on the tree builds: the only plane pairs their lowest-corner rule can be given


def _t(name):
    bc.setup(name).probe(KIND)
    T = bc.family_t(name, T_PER_CELL)
    return bc.one_per_cell(T) if name in ("dining", "so100_banana@64") else T


def _s(name):
    bc.setup(name).probe(KIND)
    S = bc.family_s(name, S_PER_CELL)
    return bc.one_per_cell(S, S_CELL) if name in ("dining", "so100_banana@64") else S


@pytest.mark.parametrize("name", SCENES + TREE_PLANES)
def test_touching_pairs_are_kept(name):
    bc.check_touching(name, KIND, _t(name))


@pytest.mark.parametrize("name", SCENES + TREE_PLANES)
def test_near_misses_are_dropped(name):
    bc.check_near_misses(name, KIND, _s(name))


@pytest.mark.parametrize("name", SCENES)
def test_real_states(name):
    xp, xm = bc.family_r(name)
    out = bc.check_batch(bc.setup(name), KIND, xp, xm, "R")
    assert out[True]["kept"].sum() > 0


@pytest.mark.parametrize("name", SCENES)
def test_over_capacity(name):
    bc.check_over_capacity(name, KIND, 4)


def test_builds_agree():
    """the ALOHA frames on the 32-dof and the 64-dof tree build: the same list bit for bit; the SO100 states on all three builds: the same
    decisions wherever the band binds them"""
    for xp, xm in (bc.family_r("aloha"), tuple(np.array([c[k] for c in _s("aloha")]) for k in ("xpos", "xmat"))):
        a, b = bc.setup("aloha").probe(KIND).run(xp, xm), bc.setup("aloha@64").probe(KIND).run(xp, xm)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1][:, :a[1].shape[1]]) and np.all(b[1][:, a[1].shape[1]:] == 0xffffffff) and np.array_equal(a[2], b[2])
    x0, m0 = bc.family_r("so100_banana")
    for other in ("so100_banana@32", "so100_banana@64"):
        x1, m1 = bc.family_r(other)
        bc.check_batch(bc.setup(other), KIND, x1, m1, "R")
        bc.check_same_decisions("so100_banana", other, KIND, x0, m0, x1, m1)
