"""Proximity sensing without a GPU: the library's argument checks, the fp64 reference against its own certificate, and the kernel source
through the emulated build (tests/hostemu) on the cases of tests/proximity_cases.py - one module-scoped fixture does all launches.  The
checks are shared with tests/test_proximity_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from so101_sim_amd import contacts as ct, native, proximity as px
from tests import contact_cases as cc, proximity_cases as pc
from tests.simharness import ArraySim


@pytest.fixture(scope="module")
def emu(blobs, golden):
    return pc.run(ArraySim(blobs["f32"], pc.N_ENVS, backend="emu"), blobs, golden)


@pytest.fixture(scope="module")
def ref(blobs, golden):
    return pc.reference(blobs, golden)


def test_argument_and_state_errors(blobs):
    pc.check_argument_errors(ArraySim(blobs["f32"], 2, backend="emu"), blobs)


def test_reference_passes_its_own_certificate(ref):
    worst = max(pc.check_reference_certificate(ref[k], ref["ref"]) for k in ("rich", "way", "single", "parallel"))
    print(f"fp64 reference against its own certificate: worst violation {worst:.3e}")


def test_separated_results_against_the_reference_and_the_certificate(emu, ref):
    pc.check_all_separated(emu, ref)


def test_penetrating_results_are_what_touch_reports(emu):
    assert pc.check_penetrating(emu["rich"], emu["touch"], emu["group_masks"], 4) >= 3


def test_own_angles_permutation_swap_and_bound_state(emu):
    pc.check_invariants(emu)


def test_a_group_is_the_minimum_of_its_members(emu):
    pc.check_members(emu)


def test_beyond_max_dist_and_outside_the_batch(emu):
    pc.check_beyond(emu)


def test_python_layer_rejects_bad_arguments(blobs):
    pc.check_python_arguments(blobs)
    assert px.ProximityReport._fields == ("dist", "geom", "point", "normal", "flags")
