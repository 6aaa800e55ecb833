"""TEST HARNESS ONLY: builds and loads plan_probe.cpp - the launch-plan functions of csrc/so101_step_plan.hpp - with the host compiler, cached
under tests/devprims/build/ by a hash of the compiler command and the two sources, the way tests/devprims/__init__.py caches its probes."""
from __future__ import annotations

import ctypes as C
import os

from tests import devprims

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_probe.cpp")
HEADER = os.path.join(devprims.CSRC, "so101_step_plan.hpp")
KNOBS = ("narrow_chunk", "narrow_chunk_light", "narrow_rows", "narrow_list_rows", "narrow_waves_q", "tree_slices", "tree_narrow_waves_q")
UNSET = dict(narrow_chunk=0, narrow_chunk_light=0, narrow_rows=-1, narrow_list_rows=-1, narrow_waves_q=0, tree_slices=0, tree_narrow_waves_q=0)


def build() -> str:
    return devprims.cached_build(SRC, "host", extra_inputs=[HEADER])


class Probe:
    def __init__(self):
        L = self.lib = C.CDLL(build())
        ip = C.POINTER(C.c_int)
        L.plan_probe_read_knobs.argtypes = [ip]
        L.plan_probe_so100.argtypes = [C.c_int] * 3 + [ip, C.c_char_p, ip, ip, ip]
        L.plan_probe_tree.argtypes = [C.c_int] * 6 + [ip, ip, ip]
        self.max_slices = L.plan_probe_max_slices()

    @staticmethod
    def _knobs(kw):
        assert set(kw) <= set(KNOBS), kw
        return (C.c_int * len(KNOBS))(*[kw.get(k, UNSET[k]) for k in KNOBS])

    def read_knobs(self) -> dict:
        """StepKnobs as read_step_knobs() finds them in the environment of this process"""
        out = (C.c_int * len(KNOBS))()
        self.lib.plan_probe_read_knobs(out)
        return dict(zip(KNOBS, out))

    def so100(self, n, groups=0, hw_queues=16, debug_bounds=None, **knobs) -> dict:
        M = self.max_slices
        head, bounds, waves = (C.c_int * 6)(), (C.c_int * (M + 1))(), (C.c_int * M)()
        self.lib.plan_probe_so100(n, groups, hw_queues, self._knobs(knobs), None if debug_bounds is None else debug_bounds.encode(), head, bounds, waves)
        G = head[0]
        assert 1 <= G <= M
        return dict(G=G, deal=head[1], rows=head[2], list_rows=head[3], narrow_chunk=head[4], bounds=list(bounds[:G + 1]), waves=list(waves[:G]))

    def tree(self, n, n_substeps=10, post=False, chain_ready=True, max_slices=4, max_sub=64, **knobs) -> dict:
        M = self.max_slices
        head, sl = (C.c_int * 2)(), (C.c_int * (3 * M))()
        self.lib.plan_probe_tree(n, n_substeps, int(post), int(chain_ready), max_slices, max_sub, self._knobs(knobs), head, sl)
        G = head[1]
        assert 1 <= G <= M
        return dict(chain=bool(head[0]), G=G, slices=[tuple(sl[3 * g:3 * g + 3]) for g in range(G)])
