"""The cone blocks of both Newton solvers, the wave primitives and the small math under the lane-thread emulation: the checks of
tests/blocks_cases.py on the g++ build of tests/devprims/blocks_probe.hip (tests/test_blocks_gpu.py runs the same checks on the MI355X)."""
import numpy as np
import pytest

from tests import blocks_cases as bc

KIND = "emu"


def test_reference_is_what_autograd_functional_gives():
    """the batched float64 reference against torch.autograd.functional.jacobian / hessian, case by case, in every zone and at every dim"""
    ref = bc.contact_reference(True)
    c = bc.contact_cases(True)
    picked = [int(np.nonzero((ref["zone"] == z) & (c["dim"] == d))[0][k]) for z in (bc.ZONE_BOTTOM, bc.ZONE_MIDDLE) for d in (3, 4, 6) for k in (0, 7)]
    picked += [int(np.nonzero((ref["zone"] == bc.ZONE_BOTTOM) & (c["dim"] == 1))[0][0])]
    for i in picked:
        s, g, H = bc.functional_reference(i, True)
        np.testing.assert_allclose(ref["cost"][i], s, rtol=1e-13)
        np.testing.assert_allclose(ref["grad"][i], g, rtol=1e-12, atol=1e-12 * np.abs(g).max())
        np.testing.assert_allclose(ref["hess"][i], H, rtol=1e-12, atol=1e-12 * np.abs(H).max())
        np.testing.assert_allclose(ref["d1"][i], g @ c["dr"][i].astype(np.float64), rtol=1e-10, atol=1e-12 * ref["d1_s"][i])
        np.testing.assert_allclose(ref["d2"][i], c["dr"][i].astype(np.float64) @ H @ c["dr"][i], rtol=1e-10, atol=1e-12 * ref["d2_s"][i])


@pytest.mark.parametrize("engine", ["so100", "tree"])
def test_contact_blocks_against_fp64(engine):
    bc.check_contact_reference(KIND, engine)


@pytest.mark.parametrize("engine", ["so100", "tree"])
def test_contact_blocks_consistent(engine):
    bc.check_contact_consistency(KIND, engine)


@pytest.mark.parametrize("engine", ["so100", "tree"])
def test_contact_rows_beyond_dim(engine):
    bc.check_contact_garbage(KIND, engine)


def test_contact_engines_agree():
    bc.check_engines_agree(KIND)


@pytest.mark.parametrize("engine", ["so100", "tree"])
def test_scalar_rows(engine):
    bc.check_rows(KIND, engine)


def test_wave_sums():
    bc.check_wave_sums(KIND)


def test_wave_extrema():
    bc.check_wave_extrema(KIND)


def test_wave_row_variants():
    bc.check_wave_rows(KIND)


def test_wave_moves():
    bc.check_wave_moves(KIND)


def test_mfma_32x32x2():
    bc.check_mfma(KIND)


def test_sincos():
    bc.check_sincos(KIND)


def test_quaternions():
    bc.check_quat(KIND)


def test_impedance():
    bc.check_impedance(KIND)


def test_rng_uniform():
    bc.check_rng(KIND)


def test_tri():
    bc.check_tri(KIND)
