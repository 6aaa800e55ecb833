"""Shared cases of the contact-interface tests (so101_contacts, include/so101.h): the raw call on an ArraySim of either backend, the
states, the group pairs, and the checks both backends run - tests/test_contacts_emu.py on 4 states through the emulated build,
tests/test_contacts_gpu.py on all 24 on the MI355X.  What does not depend on the engine serves the general-tree engine's tests as well
(tests/tree_contact_cases.py): raw_contacts, check_touch, force_errors, bound4, the frame, swap, outside and row checks.

The pairs.  `gripper | object`, `arm | table`, `fixed_jaw_pads | object`, `object | container`, `arm | arm` and `gripper | arm`, whose
groups overlap; no state of the fixture has a jaw pad on the object or the object on the container (those two pairs are the
"nobody touches" case: count 0, dist +inf, zero sums), so `fixed_jaw_pads | table` is added for a pad group with contacts.
A contact between two arm links holds BOTH orders of `arm | arm` (and a jaw-jaw contact both of `gripper | arm`): it counts once with the sign of the first order, so swapping a and b leaves its contribution as it is.  The swap check therefore
asks for the exact negation of pair_force on the pairs none of whose contacts holds both orders, and for unchanged bits on a
pair whose two groups are the same set.

The force-sum bound: 1e-5 * sum |f_k| + 1e-7 - 64 terms of fp32 summation plus a 3 x 3 rotation, a few 1e-7 relative each."""
from __future__ import annotations

import math

import numpy as np

from so101_sim_amd import contacts as ct, native
from so101_sim_amd.model import blob as blobfmt
from tests import contact_ref as cr

C = native.MAXCON
EMU_STATES = (0, 12, 16, 3)        # arm-arm in both orders + Base; jaws and wrist on the object; jaw pads, banana, bowl; a short list
FREE_STATE = 11                    # the fixture's state without any contact
PAIR_SPECS = (("gripper", "object"), ("arm", "table"), ("fixed_jaw_pads", "object"), ("object", "container"), ("arm", "arm"), ("gripper", "arm"),
              ("fixed_jaw_pads", "table"))
FIELDS = native.CONTACT_OUT_FIELDS
_PER_CONTACT = dict(geom=(2,), dist=(), pos=(3,), frame=(9,), force=(6,))          # [n, capacity] + this; count and flags are [n]
_INT = ("count", "flags", "geom", "pair_count")
GEOMETRY = ("count", "flags", "geom", "dist", "pos", "frame")
PAIR_GEOMETRY, PAIR_FORCES = ("pair_count", "pair_dist"), ("pair_normal", "pair_force")

bits = lambda a: np.ascontiguousarray(a).view(np.int32)
same_bits = lambda a, b: a.shape == b.shape and np.array_equal(bits(a), bits(b))


def groups(blobs):
    return ct.so100_groups(blobs["meta"], blobfmt.unpack(blobs["f32"]))


def pair_masks(blobs, specs=PAIR_SPECS):
    g = groups(blobs)
    return [(ct.resolve(a, g, blobs["meta"]).mask(), ct.resolve(b, g, blobs["meta"]).mask()) for a, b in specs]


def rich_states(golden, which=None):
    """-> Q [20, n], V [18, n], A [6, n], W [18, n] of tests/golden/contact_rich_states.json (`which`: indices, None = all 24)"""
    st = golden["contact_rich_states"]["states"]
    st = st if which is None else [st[i] for i in which]
    return tuple(np.array([s[k] for s in st]).T for k in ("qpos", "qvel", "action", "warm"))


def load(sim, Q, V, A, W):
    sim.set_state(Q, V, A, W)
    return sim


def raw_contacts(sim, n=None, env_index=None, forces=False, pairs=(), want=None, capacity=None):
    """so101_contacts on an ArraySim / so101_tree_contacts on a TreeArraySim -> dict of numpy arrays, the per-contact ones [n, capacity, k]
    (`capacity` None: the handle's own - a tree handle's max_contacts, else native.MAXCON).  `want`: the outputs asked for (None: everything
    the call allows).  The outputs start as 7e7 / -7, so an element the kernel does not write fails every check."""
    n = sim.N if n is None else n
    P = len(pairs)
    cap = capacity if capacity is not None else getattr(sim.sim, "max_contacts", C)
    if want is None:
        want = [k for k in FIELDS if (forces or k not in ("force",) + PAIR_FORCES) and (P or not k.startswith("pair_"))]
    gpu = sim.backend == "gpu"
    arrs = {}
    for k in want:
        if k.startswith("pair_"):
            shape = (n, P) + ((3,) if k == "pair_force" else ())
        else:
            shape = (n, cap) + _PER_CONTACT[k] if k in _PER_CONTACT else (n,)
        dt, fill = (np.int32, -7) if k in _INT else (np.float32, 7e7)
        arrs[k] = sim.torch.full(shape, fill, dtype=sim.torch.int32 if dt == np.int32 else sim.torch.float32, device=sim.dev) if gpu else np.full(shape, fill, dtype=dt)
    idx = None
    if env_index is not None:
        idx = np.ascontiguousarray(env_index, dtype=np.int32)
        idx = sim.torch.as_tensor(idx).to(sim.dev) if gpu else idx
    out = native.ContactOut(**{k: sim.ptr(a) for k, a in arrs.items()})
    sim.sim.contacts(sim.ptr(idx) if idx is not None else None, n, forces, list(pairs), out, sim.stream())
    return {k: sim._get(a) for k, a in arrs.items()}


def as_list(rep, e):
    """entry e of a raw report as the list of dicts tests.parity_cases._compare_contact_lists and Oracle.inject_contacts take"""
    k = int(rep["count"][e])
    return [dict(pos=rep["pos"][e, i].astype(np.float64), normal=rep["frame"][e, i, 0:3].astype(np.float64), dist=float(rep["dist"][e, i]),
                 geom1=int(rep["geom"][e, i, 0]), geom2=int(rep["geom"][e, i, 1])) for i in range(k)]


# ---------------------------------------------------------------------------------------------------------------- checks
def check_equals_dump(rep, geo, dbg):
    """count, geom, dist, pos, frame row 0 and force are the bits of so101_debug_forward's dump (DBG_CON, DBG_FORCE, ncon), flags its
    overflow word; slots beyond count are filled; the geometry without forces is the geometry with forces, bit for bit"""
    for e, d in enumerate(dbg):
        k = int(rep["count"][e])
        assert k == d["ncon"] == len(d["contacts"]) and int(rep["flags"][e]) == d["overflow"], (e, k, d["ncon"], rep["flags"][e], d["overflow"])
        for i, c in enumerate(d["contacts"]):
            assert (int(rep["geom"][e, i, 0]), int(rep["geom"][e, i, 1])) == (c["geom1"], c["geom2"]), (e, i)
            # (the dump is float32 widened to float64 by the harness: widening this side the same way compares the float32 bits)
            assert float(rep["dist"][e, i]) == c["dist"], (e, i)
            assert np.array_equal(rep["pos"][e, i].astype(np.float64), c["pos"]), (e, i)
            assert np.array_equal(rep["frame"][e, i, 0:3].astype(np.float64), c["normal"]), (e, i)
            assert np.array_equal(rep["force"][e, i].astype(np.float64), c["force"]), (e, i, rep["force"][e, i], c["force"])
        assert np.all(rep["geom"][e, k:] == -1) and np.all(np.isposinf(rep["dist"][e, k:]))
        assert np.all(bits(rep["pos"][e, k:]) == 0) and np.all(bits(rep["frame"][e, k:]) == 0) and np.all(bits(rep["force"][e, k:]) == 0)
    for f in ("count", "geom", "dist", "pos", "frame"):
        assert same_bits(rep[f], geo[f]), f
    # (flags: the collision's bits are those of the pass without forces; the solve may add its own)
    assert np.all((rep["flags"] & geo["flags"]) == geo["flags"])


def check_frames(rep):
    """rows orthonormal to 1e-6; rows 1 and 2 are the fp64 completion of the kernel's own row 0 to 1e-6"""
    worst_o, worst_c = 0.0, 0.0
    for e in range(len(rep["count"])):
        for i in range(max(int(rep["count"][e]), 0)):
            R = rep["frame"][e, i].astype(np.float64).reshape(3, 3)
            worst_o = max(worst_o, np.abs(R @ R.T - np.eye(3)).max())
            worst_c = max(worst_c, np.abs(R[1:] - cr.make_frame(R[0])[1:]).max())
    print(f"contact frames: worst |R R^T - I| {worst_o:.3e}, worst |rows 1, 2 - fp64 completion of row 0| {worst_c:.3e}")
    assert worst_o <= 1e-6 and worst_c <= 1e-6, (worst_o, worst_c)


def check_touch(rep, masks, k=1e-5):
    """the pair outputs of `rep` (a report with forces, pairs = masks) against the fp64 reduction of its own per-contact output; the sums
    within k * sum |f_j| + 1e-7 (the module docstring; tests/tree_contact_cases.py: SUM_BOUND_K)"""
    worst = 0.0
    seen = np.zeros(len(masks), dtype=bool)
    for e in range(len(rep["count"])):
        m = int(rep["count"][e])
        cnt, dmin, normal, net, scale = cr.reduce_pairs(masks, rep["geom"][e, :m], rep["dist"][e, :m], rep["frame"][e, :m], rep["force"][e, :m])
        assert np.array_equal(rep["pair_count"][e], cnt), (e, rep["pair_count"][e], cnt)
        assert np.array_equal(rep["pair_dist"][e].astype(np.float64), dmin), (e, rep["pair_dist"][e], dmin)
        bound = k * scale + 1e-7
        en, ef = np.abs(rep["pair_normal"][e] - normal), np.abs(rep["pair_force"][e] - net).max(axis=1)
        worst = max(worst, (np.maximum(en, ef) / bound).max())
        assert np.all(en <= bound) and np.all(ef <= bound), (e, en, ef, bound)
        seen |= cnt > 0
    print(f"touch sums vs fp64 (k = {k:g}): worst error / bound {worst:.3e}; pairs with contacts {seen.tolist()}")
    return seen


def check_swap(rep, swapped, masks):
    """a and b exchanged: counts, distances and normal sums keep their bits; pair_force is negated exactly on every pair none of whose
    contacts holds both orders, and keeps its bits where a and b are the same set"""
    for f in ("pair_count", "pair_dist", "pair_normal"):
        assert same_bits(rep[f], swapped[f]), f
    negated = 0
    for e in range(len(rep["count"])):
        k = int(rep["count"][e])
        for p, (a, b) in enumerate(masks):
            both = any(cr.both_orders(a, b, int(g1), int(g2)) for g1, g2 in rep["geom"][e, :k])
            if not both:
                assert np.array_equal(swapped["pair_force"][e, p], -rep["pair_force"][e, p]), (e, p)
                negated += int(np.any(rep["pair_force"][e, p] != 0))
            elif a == b:
                assert same_bits(swapped["pair_force"][e, p], rep["pair_force"][e, p]), (e, p)
    assert negated > 0, "no pair with a non-zero force was swapped"


def check_outside(rep, rows, npair):
    """the convention of an env_index entry outside the batch"""
    for r in rows:
        assert rep["count"][r] == -1 and rep["flags"][r] == 0 and np.all(rep["geom"][r] == -1)
        for f in ("dist", "pos", "frame", "force", "pair_dist", "pair_normal", "pair_force"):
            if f in rep:
                assert np.all(np.isnan(rep[f][r])), f
        if npair:
            assert np.all(rep["pair_count"][r] == 0)


def check_rows_equal(rep, rows, ref, ref_rows):
    """entries `rows` of `rep` carry the bits of entries `ref_rows` of `ref`, field by field (the fields both have)"""
    for f in rep:
        if f in ref:
            assert same_bits(rep[f][list(rows)], ref[f][list(ref_rows)]), f


def force_errors(rep, e, f_ref):
    """(per contact, per geom pair) error of entry e over its largest reference normal force: max over contacts and the six entries of
    |f - f_ref|, and max over the touching geom pairs of |net - net_ref|, net = sum over the pair's contacts of R^T f[0:3]"""
    k = int(rep["count"][e])
    if k == 0:
        return 0.0, 0.0
    f = rep["force"][e, :k].astype(np.float64)
    scale = f_ref[:, 0].max()
    nets, refs = {}, {}
    for i in range(k):
        key = (int(rep["geom"][e, i, 0]), int(rep["geom"][e, i, 1]))
        R = rep["frame"][e, i].astype(np.float64).reshape(3, 3)
        nets[key] = nets.get(key, 0.0) + R.T @ f[i, :3]
        refs[key] = refs.get(key, 0.0) + cr.make_frame(R[0]).T @ f_ref[i, :3]          # (the oracle completes the injected normal itself)
    return np.abs(f - f_ref).max() / scale, max(np.abs(nets[key] - refs[key]).max() for key in nets) / scale


def bound4(x):
    """4 x, rounded up to one significant digit"""
    y = 4.0 * x
    p = 10.0 ** math.floor(math.log10(y))
    return math.ceil(y / p - 1e-9) * p
