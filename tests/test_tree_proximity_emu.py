"""Proximity sensing of the general-tree engine without a GPU: so101_tree_proximity through the emulated build of the kernel source
(tests/hostemu) on the three hand-over states and, with one entry and two pairs, on the settled Dining state (tests/tree_proximity_cases.py),
against the fp64 reference of tests/tree_proximity_ref.py and the emulated so101_tree_contacts; the library's argument checks for both builds;
the Python layer's own argument checks.  The checks themselves are shared with tests/test_tree_proximity_gpu.py."""
import pytest

from tests import proximity_cases as px, tree_proximity_cases as tp
from tests.simharness import TreeArraySim


@pytest.fixture(scope="module")
def emu():
    """ONE pass of every launch the tests below read (each emulated launch costs seconds), and the fp64 side"""
    sim = TreeArraySim(tp.blobs("handover")["f32"], 3, backend="emu")
    res = tp.run_handover(sim)
    dsim = TreeArraySim(tp.blobs("dining")["f32"], 1, backend="emu")
    assert (sim.sim.build, dsim.sim.build) == (32, 64)
    return dict(res=res, ref=tp.reference("handover", res["way_adr"]), dining=tp.run_dining(dsim, 2), dref=tp.reference("dining"))


def test_separated_results_match_the_fp64_reference(emu):
    tp.check_handover_separated(emu["res"], emu["ref"])


def test_the_reference_passes_its_own_certificate(emu):
    tp.check_reference(emu["ref"], ("group", "big", "single", "way"))
    tp.check_reference(emu["dref"], ("group",))


def test_penetrating_results_are_the_contact_reports(emu):
    res = emu["res"]
    assert tp.check_penetrating(res["group"], res["touch"], res["group_masks"], 3) >= 4


def test_own_q_permutation_swap_and_untouched_state(emu):
    tp.check_invariants(emu["res"])


def test_q_moves_what_it_names_and_nothing_else(emu):
    tp.check_waypoints(emu["res"], emu["ref"])


def test_a_group_is_the_minimum_of_its_members(emu):
    tp.check_members(emu["res"])


def test_culling_spares_most_of_arms_props(emu):
    tp.check_culling(emu["res"])


def test_beyond_outside_and_nan(emu):
    px.check_beyond(emu["res"])
    assert emu["res"]["beyond"]["flags"][1, 0] == 12


def test_dining_through_the_64_dof_build(emu):
    d, worst = emu["dining"], dict(dist=0.0, cert=0.0)
    ns, npn = tp.check_separated(d["group"], [emu["dref"]["group"][0][:2]], emu["dref"]["ref"], "dining", worst)
    assert ns + npn == 2
    tp.check_penetrating(d["group"], d["touch"], d["masks"], 1)
    print(f"dining: worst |dist - reference| {worst['dist']:.3e} m, certificate {worst['cert']:.3e} m")


@pytest.mark.parametrize("kind", ["handover", "dining"])
def test_argument_and_state_errors(kind):
    tp.check_argument_errors(kind, "emu")


def test_python_layer_argument_errors():
    tp.check_python_arguments()
