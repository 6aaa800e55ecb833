"""The cone blocks of both Newton solvers, the wave primitives and the small math on the MI355X: the checks of
tests/blocks_cases.py on the gfx950 build of tests/devprims/blocks_probe.hip (tests/test_blocks_emu.py runs the same checks on the emulated build)."""
import pytest

from tests import blocks_cases as bc

KIND = "gpu"
pytestmark = pytest.mark.gpu


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
