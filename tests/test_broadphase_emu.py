"""The two broadphases against fp64 through the emulated probe builds (tests/devprims/broadphase_probe.hip with tests/hostemu): cases and checks
in tests/broadphase_cases.py, reference in tests/broadphase_ref.py.  The emulator runs about a tenth of the cases of tests/test_broadphase_gpu.py
(one per cell of families T and S, four real states and their jittered copies); the case counts of the full families are checked here with the
reference alone."""
import numpy as np
import pytest

from tests import broadphase_cases as bc

KIND = "emu"
SCENES = ("so100_banana", "so100_pen", "aloha", "dining")
T_PER_CELL, S_PER_CELL = 6, 25
S_CELL = ("type", "delta", "kind")


@pytest.mark.parametrize("name", SCENES)
def test_geoms_inside_their_boxes_and_spheres(name):
    """check 1: every geom lies inside its geom_aabb box and its geom_rbound sphere in fp64, to 1e-6 m"""
    box, sph = bc.setup(name).scene.static_violation()
    print(f"{name}: worst reach outside geom_aabb {box.max():.3e} m, outside geom_rbound {sph.max():.3e} m")
    assert box.max() <= 1e-6 and sph.max() <= 1e-6


@pytest.mark.parametrize("name", SCENES)
def test_family_t_is_certified(name):
    """the full family T with the reference alone (at the geom frames the emulated probe holds): every (type pair, delta) cell of the list, the smallest / largest / a middle hull, at most 10 % of a cell left out"""
    bc.setup(name).probe(KIND)
    bc.check_family_t(name, T_PER_CELL)


@pytest.mark.parametrize("name", SCENES)
def test_family_s_is_large_enough(name):
    """the full family S with the reference and the product's tables: at least 50 near misses per pair type, at most 5 % of a cell within the band"""
    bc.setup(name).probe(KIND)
    bc.check_family_s(name, S_PER_CELL)


TREE_PLANES = "so100_banana@32"         # the SO100 scene on a tree build: the only plane pairs the tree's lowest-corner rule can be given


@pytest.mark.parametrize("name", SCENES[:3] + (TREE_PLANES,))
def test_touching_pairs_are_kept(name):
    bc.setup(name).probe(KIND)
    bc.check_touching(name, KIND, bc.one_per_cell(bc.family_t(name, T_PER_CELL)))


@pytest.mark.parametrize("name", SCENES[:3] + (TREE_PLANES,))
def test_near_misses_are_dropped(name):
    bc.setup(name).probe(KIND)
    bc.check_near_misses(name, KIND, bc.one_per_cell(bc.family_s(name, S_PER_CELL), S_CELL))


@pytest.mark.parametrize("name", SCENES)
def test_real_states(name):
    xp, xm = bc.family_r(name, 4)
    out = bc.check_batch(bc.setup(name), KIND, xp, xm, "R")
    assert out[True]["kept"].sum() > 0


@pytest.mark.parametrize("name", SCENES[:3])
def test_over_capacity(name):
    bc.check_over_capacity(name, KIND, 2)


def test_builds_agree():
    """the ALOHA frames on the 32-dof and the 64-dof tree build: the same list bit for bit; the SO100 states on all three builds: the same
    decisions wherever the band binds them"""
    xp, xm = bc.family_r("aloha", 4)
    a, b = bc.setup("aloha").probe(KIND).run(xp, xm), bc.setup("aloha@64").probe(KIND).run(xp, xm)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1][:, :a[1].shape[1]]) and np.all(b[1][:, a[1].shape[1]:] == 0xffffffff) and np.array_equal(a[2], b[2])
    x0, m0 = bc.family_r("so100_banana", 4)
    for other in ("so100_banana@32", "so100_banana@64"):
        x1, m1 = bc.family_r(other, 4)
        bc.check_batch(bc.setup(other), KIND, x1, m1, "R")
        bc.check_same_decisions("so100_banana", other, KIND, x0, m0, x1, m1)
