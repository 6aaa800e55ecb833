"""The launch plans of the control step (csrc/so101_step_plan.hpp) as data: how many chains, where the slices are cut, whether the sorted envs
are dealt out, how many narrowphase wavefronts a slice gets, which k_narrow instance runs and how many pairs a fetch takes.  The tables below
were produced from the rules as they stood INSIDE enqueue_pipelined (so101_hip.hip) and so101_tree_step (tu_tree.hip) before the plan module
existed, transcribed into a stand-alone program: they are the parent's behaviour, not the output of the code under test.  No GPU: the header
is plain C++ and tests/devprims/plan_probe.cpp is built with the host compiler."""
import os

import pytest

from tests.devprims import plan as planprobe


@pytest.fixture(scope="module")
def probe():
    return planprobe.Probe()


def x(v, k):
    return [v] * k


# ---- SO100 engine, cfg.groups = 0, no knob set: n -> (G, deal, narrow_chunk, bounds, waves per slice)
SO100_HWQ16 = {
    1: (1, 1, 0x11, [0, 1], [16]),
    16: (1, 1, 0x11, [0, 16], [20]),
    17: (1, 1, 0x21, [0, 17], [21]),
    63: (1, 1, 0x21, [0, 63], [78]),
    64: (4, 4, 0x21, [0, 16, 32, 48, 64], x(20, 4)),
    66: (4, 1, 0x21, [0, 16, 33, 49, 66], [20, 21, 20, 21]),
    2048: (4, 4, 0x21, [0, 512, 1024, 1536, 2048], x(640, 4)),
    2049: (4, 1, 0x242, [0, 512, 1024, 1536, 2049], [640, 640, 640, 641]),
    4096: (4, 4, 0x242, [0, 1024, 2048, 3072, 4096], x(1280, 4)),
    4097: (4, 1, 0x242, [0, 1024, 2048, 3072, 4097], [1536, 1536, 1536, 1537]),
    8192: (4, 4, 0x242, [0, 2048, 4096, 6144, 8192], x(3072, 4)),
    8193: (4, 1, 0x144, [0, 2048, 4096, 6144, 8193], x(4096, 4)),
    32768: (4, 4, 0x144, [0, 8192, 16384, 24576, 32768], x(4096, 4)),
}
SO100_HWQ4 = {      # n < 64 as with 16 queues
    64: (3, 1, 0x21, [0, 16, 40, 64], [20, 30, 30]),
    4096: (3, 1, 0x242, [0, 1024, 2560, 4096], [1280, 1920, 1920]),
    8192: (3, 1, 0x242, [0, 2048, 5120, 8192], [3072, 4096, 4096]),
    32768: (3, 1, 0x144, [0, 8192, 20480, 32768], x(4096, 3)),
}
# explicit cfg.groups, 16 queues: (n, groups) -> (G, deal, bounds, waves)
SO100_GROUPS = {
    (4096, 2): (2, 2, [0, 2048, 4096], [2560, 2560]),
    (4096, 3): (3, 1, [0, 1024, 2560, 4096], [1280, 1920, 1920]),
    (4096, 5): (5, 1, [0, 819, 1638, 2457, 3276, 4096], x(1023, 4) + [1025]),
    (4096, 8): (8, 8, list(range(0, 4097, 512)), x(640, 8)),
    (4096, 9): (8, 8, list(range(0, 4097, 512)), x(640, 8)),          # capped at the eight streams a handle has
    (4095, 2): (2, 1, [0, 2047, 4095], [2558, 2560]),
    (40, 4): (1, 1, [0, 40], [50]),
}
# ---- general-tree engine, chain ready, 10 substeps, no post-step narrowphase: n -> (slices (e0, ng, nw), last_plan)
TREE = {
    1: ([(0, 1, 2)], (1, 21, 1, 2)),
    127: ([(0, 127, 254)], (1, 21, 1, 2)),
    128: ([(0, 64, 128), (64, 64, 128)], (2, 42, 2, 2)),
    511: ([(0, 255, 510), (255, 256, 512)], (2, 42, 2, 2)),
    512: ([(128 * g, 128, 256) for g in range(4)], (4, 84, 4, 2)),
    4096: ([(1024 * g, 1024, 2048) for g in range(4)], (4, 84, 4, 2)),
    16384: ([(4096 * g, 4096, 4096) for g in range(4)], (4, 84, 4, 2)),
}


def so100_invariants(p, n):
    G, b = p["G"], p["bounds"]
    assert b[0] == 0 and b[-1] == n and all(b[g] <= b[g + 1] for g in range(G)), p
    if n >= G:
        assert all(b[g] < b[g + 1] for g in range(G)), p
    assert p["deal"] in (1, G), p
    assert all(16 <= w <= 4096 for w in p["waves"]), p
    heavy, light = p["narrow_chunk"] & 15, (p["narrow_chunk"] >> 4) & 15
    assert 1 <= heavy <= 4 and 1 <= light <= 4 and p["narrow_chunk"] >> 10 == 0, p
    assert (p["narrow_chunk"] >> 8) & 1 == p["rows"] and (p["narrow_chunk"] >> 9) & 1 == p["list_rows"] and not (p["rows"] and p["list_rows"]), p


def tree_invariants(p, n):
    sl = p["slices"]
    assert sl[0][0] == 0 and sum(ng for _, ng, _ in sl) == n and all(a[0] + a[1] == b[0] for a, b in zip(sl, sl[1:])), p
    if n >= p["G"]:
        assert all(ng > 0 for _, ng, _ in sl), p
    if p["chain"]:
        assert all(1 <= nw <= 4096 for _, _, nw in sl), p


def tree_last_plan(p, n_substeps=10, post=False):
    """so101_tree_last_plan as so101_tree_step counts it while it executes the plan: per slice one memset, the prologue, two launches per
    substep and two more for the post-step narrowphase; the single kernel is one launch"""
    if not p["chain"]:
        return (1, 1, 0, 1)
    return (p["G"], p["G"] * (1 + 2 * n_substeps + (2 if post else 0)), p["G"], 2)


@pytest.mark.parametrize("hwq,table", [(16, SO100_HWQ16), (4, SO100_HWQ4), (4, {n: v for n, v in SO100_HWQ16.items() if n < 64})])
def test_so100_plan_tables(probe, hwq, table):
    for n, (G, deal, chunk, bounds, waves) in table.items():
        p = probe.so100(n, hw_queues=hwq)
        assert (p["G"], p["deal"], p["narrow_chunk"], p["bounds"], p["waves"]) == (G, deal, chunk, bounds, waves), (n, hwq, p)
        so100_invariants(p, n)
    # the threshold between three and four chains: six queues
    assert probe.so100(4096, hw_queues=5)["G"] == 3 and probe.so100(4096, hw_queues=6)["G"] == 4


def test_so100_plan_with_explicit_groups(probe):
    for (n, groups), (G, deal, bounds, waves) in SO100_GROUPS.items():
        p = probe.so100(n, groups=groups)
        assert (p["G"], p["deal"], p["bounds"], p["waves"]) == (G, deal, bounds, waves), (n, groups, p)
        so100_invariants(p, n)
    # explicit groups do not ask the queues
    assert probe.so100(4096, groups=4, hw_queues=4) == probe.so100(4096, hw_queues=16)


def test_so100_plan_knobs(probe):
    # SO101_NARROW_ROWS=1: the row pass (bit 8) at any size, and never the list row pass beside it (bit 9); chunks as without it
    p = probe.so100(8, narrow_rows=1)
    assert p["narrow_chunk"] == 0x100 | 0x11 and p["rows"] == 1 and p["list_rows"] == 0
    assert probe.so100(8, narrow_rows=1, narrow_list_rows=1)["narrow_chunk"] == 0x100 | 0x11
    assert probe.so100(32768, narrow_rows=0)["narrow_chunk"] == 0x200 | 0x44          # (off above 8192 envs: the list row pass takes over)
    # SO101_NARROW_LIST_ROWS=1: bit 9, four light pairs per fetch; one heavy pair (two only where the pass is on by default, above 2048 envs)
    p = probe.so100(8, narrow_list_rows=1)
    assert p["narrow_chunk"] == 0x200 | 0x41 and p["list_rows"] == 1
    # SO101_NARROW_LIST_ROWS=0 at 4096 envs: the plan of the sizes below 2049
    assert probe.so100(4096, narrow_list_rows=0)["narrow_chunk"] == 0x21
    # SO101_NARROW_CHUNK / _LIGHT: pairs per fetch, heavy in bits 0-3, light in bits 4-7
    assert probe.so100(4096, narrow_chunk=3)["narrow_chunk"] == 0x200 | 0x43
    assert probe.so100(64, narrow_chunk=3)["narrow_chunk"] == 0x23
    assert probe.so100(64, narrow_chunk_light=4)["narrow_chunk"] == 0x41
    # SO101_NARROW_WAVES_Q=8: two wavefronts per env of the slice, still within 16 .. 4096
    assert probe.so100(4096, narrow_waves_q=8)["waves"] == x(2048, 4)
    assert probe.so100(4, narrow_waves_q=8)["waves"] == [16] and probe.so100(32768, narrow_waves_q=12)["waves"] == x(4096, 4)
    # out of range: ignored
    base = probe.so100(4096)
    for bad in (dict(narrow_chunk=0), dict(narrow_chunk=5), dict(narrow_chunk=-1), dict(narrow_chunk_light=5), dict(narrow_chunk_light=-3),
                dict(narrow_waves_q=0), dict(narrow_waves_q=-4), dict(narrow_rows=-1), dict(narrow_rows=-7), dict(narrow_list_rows=-2),
                dict(tree_slices=3), dict(tree_narrow_waves_q=16)):
        assert probe.so100(4096, **bad) == base, bad
    # nothing else moves with a knob: chains, slices and the deal are those of the table
    for kn in (dict(narrow_rows=1), dict(narrow_list_rows=1), dict(narrow_chunk=3), dict(narrow_waves_q=8)):
        p = probe.so100(66, **kn)
        assert (p["G"], p["deal"], p["bounds"]) == (4, 1, [0, 16, 33, 49, 66]), kn


def test_so100_debug_bounds_of_profiling_builds(probe):
    """SO101_DEBUG_BOUNDS (read in SO101_DEBUG_CLOCKS builds only): the ascending values below n are the slice ends"""
    p = probe.so100(4096, debug_bounds="128,1024")
    assert (p["G"], p["deal"], p["bounds"], p["waves"]) == (3, 1, [0, 128, 1024, 4096], [160, 1120, 3840])
    p = probe.so100(4096, debug_bounds="2048")
    assert (p["G"], p["deal"], p["bounds"]) == (2, 2, [0, 2048, 4096])
    assert probe.so100(4096, debug_bounds="500,400,5000,600")["bounds"] == [0, 500, 600, 4096]
    assert probe.so100(4096, debug_bounds="")["bounds"] == [0, 4096]
    so100_invariants(probe.so100(4096, debug_bounds="1,2,3,4,5,6,7,8,9,10"), 4096)


def test_knobs_are_read_from_the_environment(probe, monkeypatch):
    names = {"narrow_chunk": "SO101_NARROW_CHUNK", "narrow_chunk_light": "SO101_NARROW_CHUNK_LIGHT", "narrow_rows": "SO101_NARROW_ROWS",
             "narrow_list_rows": "SO101_NARROW_LIST_ROWS", "narrow_waves_q": "SO101_NARROW_WAVES_Q", "tree_slices": "SO101_TREE_SLICES",
             "tree_narrow_waves_q": "SO101_TREE_NARROW_WAVES_Q"}
    for v in names.values():
        monkeypatch.delenv(v, raising=False)
    assert probe.read_knobs() == planprobe.UNSET
    for k, (knob, var) in enumerate(names.items()):
        monkeypatch.setenv(var, str(k + 1))
        assert probe.read_knobs() == dict(planprobe.UNSET, **{knob: k + 1}), var          # read again at every call, and only its own variable
        monkeypatch.delenv(var)
    monkeypatch.setenv("SO101_NARROW_ROWS", "0")
    assert probe.read_knobs()["narrow_rows"] == 0
    # not a profiling build: SO101_DEBUG_BOUNDS is not read (a plan from these knobs is the plain one)
    monkeypatch.setenv("SO101_DEBUG_BOUNDS", "128,1024")
    assert "SO101_DEBUG_BOUNDS" in os.environ and probe.read_knobs() == dict(planprobe.UNSET, narrow_rows=0)


def test_tree_plan_tables(probe):
    for n, (slices, last_plan) in TREE.items():
        p = probe.tree(n)
        assert p["chain"] and p["slices"] == slices and tree_last_plan(p) == last_plan, (n, p)
        tree_invariants(p, n)
    # contact rewards: one more narrowphase launch and k_tree_pipe_finish per slice
    p = probe.tree(128, post=True)
    assert p["slices"] == TREE[128][0] and tree_last_plan(p, post=True) == (2, 46, 2, 2)
    # the work list has max_sub slots, the post-step narrowphase takes one; no chain buffers: the single kernel
    for p in (probe.tree(128, n_substeps=64, post=True), probe.tree(128, n_substeps=65), probe.tree(128, chain_ready=False), probe.tree(4096, chain_ready=False, post=True)):
        assert not p["chain"] and p["G"] == 1 and tree_last_plan(p) == (1, 1, 0, 1), p
    assert probe.tree(128, n_substeps=64)["chain"] and probe.tree(128, n_substeps=63, post=True)["chain"]
    assert probe.tree(4096, chain_ready=False)["slices"] == [(0, 4096, 0)]


def test_tree_plan_knobs(probe):
    p = probe.tree(512, tree_slices=3)
    assert p["slices"] == [(0, 170, 340), (170, 171, 342), (341, 171, 342)]
    tree_invariants(p, 512)
    assert probe.tree(512, tree_slices=5) == probe.tree(512) and probe.tree(512, tree_slices=-1) == probe.tree(512)
    assert probe.tree(512, tree_slices=1)["slices"] == [(0, 512, 1024)]
    assert probe.tree(127, tree_slices=4)["G"] == 1                    # (below 128 envs: one slice whatever is asked for)
    assert probe.tree(512, tree_narrow_waves_q=4)["slices"] == [(128 * g, 128, 128) for g in range(4)]
    assert probe.tree(512, tree_narrow_waves_q=0) == probe.tree(512) and probe.tree(512, narrow_waves_q=4, narrow_chunk=3, narrow_rows=1) == probe.tree(512)


def test_plan_invariants_for_every_small_batch(probe):
    for n in range(1, 301):
        for hwq in (4, 16):
            so100_invariants(probe.so100(n, hw_queues=hwq), n)
        for groups in (2, 5, 8):
            so100_invariants(probe.so100(n, groups=groups), n)
        for post in (False, True):
            tree_invariants(probe.tree(n, post=post), n)
        tree_invariants(probe.tree(n, tree_slices=3), n)
    # the plan functions are pure: the same arguments give the same plan, whatever was asked before
    assert probe.so100(66) == probe.so100(66) and probe.tree(511) == probe.tree(511)
