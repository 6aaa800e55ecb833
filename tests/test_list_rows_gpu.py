"""MI355X: the list row pass of k_narrow<false> (four list-backed flat-face pairs per wavefront, SO101_NARROW_LIST_ROWS) - the probe of
tests/list_rows_cases.py in full, the launch chains with the pass on against the fused step, and two handles with the pass off and on."""
import os

import numpy as np
import pytest

from tests import list_rows_cases as lc
from tests import parity_cases as pc
from tests.devprims import list_rows
from tests.simharness import ArraySim

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def make_sim(blobs):
    def f(n, seed=0, **cfg):
        return ArraySim(blobs["f32"], n, backend="gpu", seed=seed, **cfg)
    return f


def test_list_rows_probe(blobs):
    gpu = list_rows.Probes("gpu")
    seen, refused = {}, 0
    for name, V in lc.hulls(blobs).items():
        hist, r = lc.check_hull(gpu, V, name, lc.LENGTHS + (33,), tie=name in ("cube:8", "grid5:98"))
        refused += r
        for k, v in hist.items():
            seen[k] = seen.get(k, 0) + v
    assert all(seen.get(n, 0) >= 3 for n in lc.LENGTHS), seen      # (five poses settle per cell; the two tilted ones may land in a neighbour cell)
    assert refused >= 5, refused


@pytest.mark.parametrize("n,steps", [(8, 6), (512, 4)])
def test_list_row_pass_matches_fused(make_sim, golden, monkeypatch, n, steps):
    monkeypatch.setenv("SO101_NARROW_LIST_ROWS", "1")
    pc.check_pipeline_identical(make_sim, golden, n=n, steps=steps, seed=11, all_reset_last=(n == 8), pipelines=(0, 1))


def test_list_row_pass_changes_nothing_downstream(blobs):
    """Two handles, the pass off and on (the switch is read when a handle enqueues its step), the same seed and random actions across a time
    limit: states and task outputs bit for bit."""
    n, steps = 256, 16
    rng = np.random.RandomState(4)
    lo = np.array([-np.pi, -3.14158, -3.14158, -3.14158, -3.14158, 0.0], dtype=np.float32)
    hi = np.array([np.pi, 3.14158, 3.14158, 3.14158, 3.14158, 0.08], dtype=np.float32)
    acts = rng.uniform(lo, hi, size=(steps, n, 6)).astype(np.float32)
    traces, flags = [], []
    for switch in ("0", "1"):
        os.environ["SO101_NARROW_LIST_ROWS"] = switch
        try:
            sim = ArraySim(blobs["f32"], n, backend="gpu", seed=3, last_step=12, settle_max_substeps=200)
            sim.reset()
            tr = []
            for t in range(steps):
                obs, rew, disc, st = sim.step(acts[t])
                tr.append(np.concatenate([obs.ravel(), rew, disc, st.astype(np.float32)] + [a.ravel() for a in sim.get_state()]))
            flags.append(sim.sim.info()["narrow_list_rows"])
        finally:
            os.environ.pop("SO101_NARROW_LIST_ROWS", None)
        traces.append(tr)
    assert flags == [0, 1], flags
    for t, (a, b) in enumerate(zip(*traces)):
        assert np.all(np.isfinite(a))
        np.testing.assert_array_equal(a, b, err_msg=f"step {t}")
