"""Seeded cases, fp64 references, a numpy model of the wave primitives and the checks of tests/test_blocks_emu.py and tests/test_blocks_gpu.py.

Three layers that the solution-level comparisons cannot see, probed through tests/devprims/blocks_probe.hip:
  A. the per-contact cone blocks and scalar rows of both Newton solvers.  Reference: the scalar cost s(r) alone is written by hand, zone-wise,
     in float64 (MuJoCo's elliptic cone: top zone 0, bottom zone 1/2 sum D_j r_j^2, middle zone 1/2 D_m (N - mu T)^2, D_m = D_0 / (mu^2 (1 + mu^2)));
     force, Hessian and the derivatives along r + alpha dr are torch autograd of it in float64 on the CPU, never the kernels' closed forms.
  B. the wave primitives: ONE numpy float32 model per primitive, to which the gfx950 build (wave.hpp) and the emulation (tests/hostemu/wave_emu.hpp)
     are both compared.
  C. so101_math.hpp against float64 numpy, and rng_uniform against a Python-integer Philox4x32-10.

Bounds that are neither exact nor derivable are ten times what scripts/measure_block_bounds.py measures for a float32 numpy restatement of the
formulas on these same cases (the restatement, never the code under test); the measured worst stands beside each constant, and the worst the
MI355X build itself showed beside that.  Errors of force, Hessian and line derivatives are normalised by the same quantity of the cost with the
cancellation taken out, s+(r) = 1/2 D_m (|N| + mu T)^2, so that a bound does not depend on how near a zone boundary a case lies.
"""
from __future__ import annotations

import functools

import numpy as np

F = np.float32
EPS = float(np.finfo(np.float32).eps)          # 2^-23
MINVAL, MINIMP, MAXIMP = 1e-15, 1e-4, 0.9999
GARBAGE = 3.0

# ---- bounds: measured worst of the float32 restatement (scripts/measure_block_bounds.py) x 10 | worst of the MI355X build
CON_COST = 3.7e-06       # |cost - ref| / s+                                 restatement 3.720e-07 | MI355X 3.416e-07
CON_FORCE = 3.2e-06      # |force - ref|_2 / |grad s+|_2                     restatement 3.152e-07 | MI355X 2.741e-07
CON_HESS = 3.5e-05       # |Hc - ref|_F / |hess s+|_F                        restatement 3.538e-06 | MI355X 3.538e-06 (so100 against tree: 4.260e-06)
CON_D1 = 2.8e-06         # |d1 - ref| / sum_j |grad s+_j dr_j|               restatement 2.847e-07 | MI355X 2.345e-07 (contact_line against -force . dr: 2.386e-07)
CON_D2 = 2.2e-05         # |d2 - ref| / sum_jk |hess s+_jk dr_j dr_k|        restatement 2.212e-06 | MI355X 2.266e-06 (contact_line against dr' Hc dr: 2.700e-06)
QUAT2MAT = 1.4e-06       # max |entry - ref|, unit quaternions               restatement 1.419e-07 | MI355X 1.184e-07
MULQUAT = 9.9e-07        # max |entry - ref|, unit quaternions               restatement 9.908e-08 | MI355X 9.970e-08
NORMQUAT = 6.9e-07       # max |entry - ref|                                 restatement 6.897e-08 | MI355X 1.262e-07
NORMALIZE3 = 1.2e-06     # max |entry - ref|, and |norm - ref| / ref         restatement 1.194e-07 | MI355X 1.256e-07
ROTSYM = 2.0e-06         # max |entry - ref| / max |s|                       restatement 2.010e-07 | MI355X 2.010e-07
MAT2QUAT = 1.3e-06       # max |entry -+ ref|                                restatement 1.294e-07 | MI355X 1.620e-07
ROTVECQUAT = 1.9e-06     # max |entry - ref| / |v|                           restatement 1.882e-07 | MI355X 1.401e-07
IMPEDANCE = 1.0e-06      # |d - ref|                                         restatement 1.044e-07 | MI355X 9.462e-08
# derivable / the project's own
SINCOS_ULP = 2.0        # so101_math.hpp, DESIGN.md section 3.1: <= 2 ulp for |x| < 1e4            MI355X sin 1.522, cos 1.548 (the emulated build: the same)
# scalar rows: D = 1 / R is a v_rcp-based division (<= 2.5 ulp, so101_sim_amd/build.py FLAGS), then at most three roundings of half an ulp each
# (fma contraction only removes some); an ulp is at most 2^-23 relative.  Relative to the terms before any cancellation.
ROW_REL = 4.0 * EPS           # MI355X 1.467e-07
MFMA_CALLS = 18
_n = 2 * MFMA_CALLS + 1
MFMA_GAMMA = _n * EPS / (1.0 - _n * EPS)        # gamma_n of n = 2 * 18 + 1 operations on each accumulator; MI355X 5.399e-07


def worst(name, value, bound):
    """prints every figure before it is asserted (pytest -s, and the measuring scripts)"""
    print(f"  {name}: worst {value:.3e} (bound {bound:.3e})")
    return value


# ============================================================================================ A. cone blocks
DIMS = (1, 3, 4, 6)
FR_LO = np.array([0.2, 0.2, 1e-3, 1e-4, 1e-4])
FR_HI = np.array([1.5, 1.5, 0.1, 1e-2, 1e-2])
ZONE_TOP, ZONE_BOTTOM, ZONE_MIDDLE = 0, 1, 2
# where a case lies: (zone it is built for, N as a function of the boundaries)
PLACES = ["top", "middle", "bottom", "top+1e-3", "top-1e-3", "top+1e-2", "top-1e-2", "bot+1e-3", "bot-1e-3", "bot+1e-2", "bot-1e-2",
          "T0N-", "T0N0", "T0N+", "on_top", "on_bottom"]


def _loguniform(rng, lo, hi, size):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size))


@functools.lru_cache(maxsize=None)
def contact_cases(with_dim0=False):
    """dict of float32 / int32 arrays: dim, mu, fr (n, 5), D (n, 6), r (n, 6), dr (n, 6) with ZEROS in the rows >= dim, and place (index into
    PLACES).  4000 cases (4096 with the dropped contacts of the SO100 engine): one launch."""
    rng = np.random.RandomState(20240)
    per = 250                                   # per place
    out = {k: [] for k in ("dim", "mu", "fr", "D", "r", "dr", "place")}
    for p, place in enumerate(PLACES):
        for c in range(per):
            dim = DIMS[c % 4] if not place.startswith("on_") else 3
            if dim == 1 and not place.startswith("T0"):
                dim = (3, 4, 6)[c % 3]          # (a frictionless contact has no cone: it takes the T = 0 places, below)
            mu = rng.uniform(0.05, 2.0)
            fr = rng.uniform(FR_LO, FR_HI)
            D = _loguniform(rng, 1.0, 1e8, 6)
            r = np.zeros(6)
            t = rng.normal(size=5)
            if c % 2:
                t = t / fr                       # every friction row contributes alike to T (otherwise the tangential rows dominate)
            t[dim - 1:] = 0.0
            if place.startswith("on_"):
                # one tangential row, friction 1, mu = 0.5: r0 = r1 on the top boundary, r0 = -4 |r1| on the bottom one, powers of two
                mu, fr = 0.5, np.array([1.0, 1.0, fr[2], fr[3], fr[4]])
                r1 = 2.0 ** rng.randint(-2, 4) * (1 if c % 2 else -1)
                r[1] = r1
                r[0] = abs(r1) if place == "on_top" else -4.0 * abs(r1)
            elif place.startswith("T0"):
                r[0] = {"T0N-": -1.0, "T0N0": 0.0, "T0N+": 1.0}[place] * _loguniform(rng, 1e-3, 1e2, 1)[0]
            else:
                T = np.sqrt(np.sum((t * fr) ** 2))
                top, bot = mu * T, -T / mu
                if place == "top":
                    N = top * (1.0 + _loguniform(rng, 0.1, 10.0, 1)[0])
                elif place == "bottom":
                    N = bot * (1.0 + _loguniform(rng, 0.1, 10.0, 1)[0])
                elif place == "middle":
                    N = bot + rng.uniform(0.1, 0.9) * (top - bot)
                else:
                    d = float(place[3:])
                    N = top * (1.0 + d) if place.startswith("top") else bot * (1.0 - d)
                r[1:] = t
                r[0] = N / mu
                r *= _loguniform(rng, 1e-3, 1e2, 1)[0] / np.linalg.norm(r)       # (the zones are cones: scaling keeps the place)
            dr = rng.normal(size=6) * (np.linalg.norm(r) + 1e-3) * _loguniform(rng, 1e-2, 10.0, 1)[0]
            if c % 2:
                dr[1:] = dr[1:] / fr
            dr[dim:] = 0.0
            for k, v in zip(out, (dim, mu, fr, D, r, dr, p)):
                out[k].append(v)
    if with_dim0:
        for c in range(96):
            for k, v in zip(out, (0, rng.uniform(0.05, 2.0), rng.uniform(FR_LO, FR_HI), _loguniform(rng, 1.0, 1e8, 6), np.zeros(6), np.zeros(6), 0)):
                out[k].append(v)
    res = {k: np.asarray(v, dtype=np.int32 if k in ("dim", "place") else F) for k, v in out.items()}
    for v in res.values():
        v.setflags(write=False)
    return res


def with_garbage(cases):
    """the same cases with finite garbage in every row >= dim of r, dr, D and the friction array"""
    g = {k: v.copy() for k, v in cases.items()}
    rows = np.arange(6)[None, :] >= cases["dim"][:, None]
    for k in ("r", "dr", "D"):
        g[k][rows] = GARBAGE
    g["fr"][rows[:, 1:]] = GARBAGE
    return g


def zone64(c):
    """the zone of each case, decided in float64 from the float32 inputs"""
    dim, mu, r = c["dim"], c["mu"].astype(np.float64), c["r"].astype(np.float64)
    mask = np.arange(1, 6)[None, :] < dim[:, None]
    T = np.sqrt(np.sum((r[:, 1:] * c["fr"].astype(np.float64) * mask) ** 2, axis=1))
    N = mu * r[:, 0]
    top = (dim == 0) | (N >= mu * T) | ((T <= 0) & (N >= 0))
    bottom = ~top & ((mu * N + T <= 0) | ((T <= 0) & (N < 0)))
    return np.where(top, ZONE_TOP, np.where(bottom, ZONE_BOTTOM, ZONE_MIDDLE))


def _cost_t(zone, plus=False):
    """the hand-written float64 cost of one zone as a torch function of r (n, 6); plus: with |N| + mu T in place of N - mu T"""
    import torch

    def f(r, mu, fr, D, mask):
        if zone == ZONE_TOP:
            return 0.0 * r.sum(dim=1)
        if zone == ZONE_BOTTOM:
            return 0.5 * (D * mask * r * r).sum(dim=1)
        T = torch.sqrt((((r[:, 1:] * fr) ** 2) * mask[:, 1:]).sum(dim=1))
        N = mu * r[:, 0]
        Dm = D[:, 0] / (mu * mu * (1.0 + mu * mu))
        s = (torch.abs(N) + mu * T) if plus else (N - mu * T)
        return 0.5 * Dm * s * s
    return f


def _derivs(f, r, dr, args):
    """cost, gradient, Hessian and the first two derivatives of alpha -> f(r + alpha dr) at 0, all by autograd in float64"""
    import torch
    n = len(r)
    r = r.clone().requires_grad_(True)
    s = f(r, *args)
    g, = torch.autograd.grad(s.sum(), r, create_graph=True)
    H = torch.zeros(n, 6, 6, dtype=torch.float64)
    for k in range(6):
        H[:, k, :], = torch.autograd.grad(g[:, k].sum(), r, retain_graph=True)
    a = torch.zeros(n, dtype=torch.float64, requires_grad=True)
    phi = f(r.detach() + a[:, None] * dr, *args)
    d1, = torch.autograd.grad(phi.sum(), a, create_graph=True)
    d2, = torch.autograd.grad(d1.sum(), a)
    return [x.detach().numpy() for x in (s, g, H, d1, d2)]


def _torch_args(c, sel):
    import torch
    t = lambda a: torch.tensor(np.asarray(a[sel], dtype=np.float64))           # noqa: E731
    mask = (np.arange(6)[None, :] < c["dim"][sel][:, None]).astype(np.float64)
    return t(c["r"]) * torch.tensor(mask), t(c["dr"]) * torch.tensor(mask), (t(c["mu"]), t(c["fr"]), t(c["D"]), torch.tensor(mask))


@functools.lru_cache(maxsize=None)
def contact_reference(with_dim0=False):
    """float64: zone, cost, grad, hess, d1, d2 of every case of contact_cases(), and the scales of the errors (module docstring): cost_s, grad_s
    (2-norm), hess_s (Frobenius), d1_s, d2_s.  In the top zone everything is exactly zero."""
    c = contact_cases(with_dim0)
    n = len(c["dim"])
    zone = zone64(c)
    ref = dict(zone=zone, cost=np.zeros(n), grad=np.zeros((n, 6)), hess=np.zeros((n, 6, 6)), d1=np.zeros(n), d2=np.zeros(n),
               cost_s=np.ones(n), grad_s=np.ones(n), hess_s=np.ones(n), d1_s=np.ones(n), d2_s=np.ones(n))
    for z in (ZONE_BOTTOM, ZONE_MIDDLE):
        sel = np.nonzero(zone == z)[0]
        r, dr, args = _torch_args(c, sel)
        for plus in (False, True):
            s, g, H, d1, d2 = _derivs(_cost_t(z, plus), r, dr, args)
            if not plus:
                ref["cost"][sel], ref["grad"][sel], ref["hess"][sel], ref["d1"][sel], ref["d2"][sel] = s, g, H, d1, d2
            else:
                drn = dr.numpy()
                ref["cost_s"][sel], ref["grad_s"][sel] = s, np.linalg.norm(g, axis=1)
                ref["hess_s"][sel] = np.linalg.norm(H.reshape(-1, 36), axis=1)
                ref["d1_s"][sel] = np.sum(np.abs(g * drn), axis=1)
                ref["d2_s"][sel] = np.sum(np.abs(H * drn[:, :, None] * drn[:, None, :]), axis=(1, 2))
    for v in ref.values():
        v.setflags(write=False)
    return ref


def functional_reference(i, with_dim0=False):
    """cost, gradient and Hessian of case i through torch.autograd.functional, one case at a time: what contact_reference() batches"""
    import torch
    c, zone = contact_cases(with_dim0), zone64(contact_cases(with_dim0))
    r, _, args = _torch_args(c, np.array([i]))
    f = lambda x: _cost_t(int(zone[i]))(x[None, :], *args)[0]                   # noqa: E731
    return (float(f(r[0])), torch.autograd.functional.jacobian(f, r[0]).numpy(), torch.autograd.functional.hessian(f, r[0]).numpy())


def contact_errors(got, ref, sel=None):
    """normalised errors of one engine's outputs (dict of cost, force, Hc (n, 6, 6), d1, d2) against the reference: dict of per-case arrays"""
    sel = slice(None) if sel is None else sel
    e = {}
    e["cost"] = np.abs(got["cost"][sel] - ref["cost"][sel]) / ref["cost_s"][sel]
    e["force"] = np.linalg.norm(got["force"][sel].astype(np.float64) + ref["grad"][sel], axis=1) / ref["grad_s"][sel]
    e["hess"] = np.linalg.norm((got["Hc"][sel] - ref["hess"][sel]).reshape(-1, 36), axis=1) / ref["hess_s"][sel]
    e["d1"] = np.abs(got["d1"][sel] - ref["d1"][sel]) / ref["d1_s"][sel]
    e["d2"] = np.abs(got["d2"][sel] - ref["d2"][sel]) / ref["d2_s"][sel]
    return e


CON_BOUNDS = {"cost": "CON_COST", "force": "CON_FORCE", "hess": "CON_HESS", "d1": "CON_D1", "d2": "CON_D2"}


def _run_contacts(P, engine, c):
    fn = P.so100_contact if engine == "so100" else P.tree_contact
    return fn(c["dim"], c["mu"], c["fr"], c["D"], c["r"], c["dr"])


@functools.lru_cache(maxsize=None)
def probes(kind):
    from tests.devprims import blocks
    return blocks.Probes(kind)


@functools.lru_cache(maxsize=None)
def contact_outputs(kind, engine):
    """(outputs on the cases, outputs on the cases with garbage in the rows >= dim): one launch each, shared by the checks"""
    c = contact_cases(engine == "so100")
    return _run_contacts(probes(kind), engine, c), _run_contacts(probes(kind), engine, with_garbage(c))


def check_contact_reference(kind, engine):
    c, ref = contact_cases(engine == "so100"), contact_reference(engine == "so100")
    got, _ = contact_outputs(kind, engine)
    active = ref["zone"] != ZONE_TOP
    for z in (ZONE_TOP, ZONE_BOTTOM, ZONE_MIDDLE):
        assert np.sum(ref["zone"] == z) >= 500, "cases"
    # top zone and dropped contacts: exactly zero, every output
    for k in ("cost", "force", "Hc", "d1", "d2"):
        assert not np.any(got[k][~active]), k
    if engine == "so100":
        np.testing.assert_array_equal(got["zone"], ref["zone"])
        on = c["place"] >= PLACES.index("on_top")
        assert np.array_equal(got["zone"][on], np.where(c["place"][on] == PLACES.index("on_top"), ZONE_TOP, ZONE_BOTTOM))
    else:
        assert np.all((got["cost"] != 0) == (ref["cost"] != 0))
    assert np.all(np.isfinite(np.concatenate([got[k].ravel() for k in ("cost", "force", "Hc", "d1", "d2")])))
    e = contact_errors(got, ref, active)
    bad = []
    for k, name in CON_BOUNDS.items():
        b = globals()[name]
        if not worst(f"{kind} {engine} {k}", float(e[k].max()), b) <= b:
            bad.append((k, float(e[k].max()), int(np.nonzero(active)[0][np.argmax(e[k])])))
    assert not bad, bad


def check_contact_consistency(kind, engine):
    """want_h off == want_h on for cost and force; contact_line against force and Hessian of the block function; symmetry"""
    ref = contact_reference(engine == "so100")
    c = contact_cases(engine == "so100")
    got, _ = contact_outputs(kind, engine)
    np.testing.assert_array_equal(got["cost"].view(np.uint32), got["cost0"].view(np.uint32))
    np.testing.assert_array_equal(got["force"].view(np.uint32), got["force0"].view(np.uint32))
    if engine == "so100":
        np.testing.assert_array_equal(got["zone"], got["zone0"])
    else:
        np.testing.assert_array_equal(got["Hc"].view(np.uint32), got["Hc"].transpose(0, 2, 1).view(np.uint32))
    dr = c["dr"].astype(np.float64)
    d1 = -np.sum(got["force"] * dr, axis=1)
    d2 = np.einsum("nj,njk,nk->n", dr, got["Hc"].astype(np.float64), dr)
    e1, e2 = np.abs(got["d1"] - d1) / ref["d1_s"], np.abs(got["d2"] - d2) / ref["d2_s"]
    assert worst(f"{kind} {engine} line d1 vs -force . dr", float(e1.max()), CON_D1) <= CON_D1, int(np.argmax(e1))
    assert worst(f"{kind} {engine} line d2 vs dr' Hc dr", float(e2.max()), CON_D2) <= CON_D2, int(np.argmax(e2))


def check_contact_garbage(kind, engine):
    """rows >= dim: zero outputs, and nothing else moves by a bit when their inputs do"""
    c = contact_cases(engine == "so100")
    got, gar = contact_outputs(kind, engine)
    for k in got:
        np.testing.assert_array_equal(got[k].view(np.uint32) if got[k].dtype == F else got[k], gar[k].view(np.uint32) if gar[k].dtype == F else gar[k], err_msg=k)
    rows = np.arange(6)[None, :] >= c["dim"][:, None]
    for o in (got, gar):
        assert not np.any(o["force"][rows]) and not np.any(o["force0"][rows])
        assert not np.any(o["Hc"][rows]) and not np.any(o["Hc"].transpose(0, 2, 1)[rows])


def check_engines_agree(kind):
    """SO100's packed Hessian and the tree's full one on the same inputs (the first 4000 cases are shared)"""
    ref = contact_reference(False)
    a, b = contact_outputs(kind, "so100")[0], contact_outputs(kind, "tree")[0]
    n = len(ref["zone"])
    e = np.linalg.norm((a["Hc"][:n].astype(np.float64) - b["Hc"]).reshape(n, 36), axis=1) / ref["hess_s"]
    assert worst(f"{kind} Hc so100 vs tree", float(e.max()), CON_HESS) <= CON_HESS, int(np.argmax(e))
    f = np.linalg.norm(a["force"][:n].astype(np.float64) - b["force"], axis=1) / ref["grad_s"]
    assert worst(f"{kind} force so100 vs tree", float(f.max()), CON_FORCE) <= CON_FORCE, int(np.argmax(f))


# ---- scalar rows
TR_FRICTION, TR_LIMIT, TR_EQUALITY = 0, 1, 3


@functools.lru_cache(maxsize=None)
def row_cases():
    """type, R, floss, jar (float32).  R and floss carry few mantissa bits where a case sits at or next to +-R floss, so that the product
    is exact in float32 and in float64."""
    rng = np.random.RandomState(77)
    T, R, fl, jar = [], [], [], []
    for c in range(1200):
        t = (TR_FRICTION, TR_LIMIT, TR_EQUALITY)[c % 3]
        Rv = rng.randint(1, 256) / 2.0 ** rng.randint(4, 20)
        flv = rng.randint(1, 256) / 64.0 if t == TR_FRICTION else 0.0
        k = (c // 3) % 8
        if t == TR_FRICTION:
            rf = Rv * flv
            j = [rf, -rf, rf * (1 + 1e-3), rf * (1 - 1e-3), -rf * (1 + 1e-3), -rf * (1 - 1e-3), rng.normal() * rf, rng.normal() * 10 * rf][k]
        else:
            j = [0.0, -0.0, 1.0, -1.0][k % 4] * _loguniform(rng, 1e-3, 1e2, 1)[0]
        T.append(t); R.append(Rv); fl.append(flv); jar.append(j)
    return np.array(T, np.int32), np.array(R, F), np.array(fl, F), np.array(jar, F)


def row_reference(T, R, fl, jar):
    """float64 cost by hand; force = -ds/djar and h = d2s/djar2 by autograd.  Returns cost, force, h and the scale of the cost's terms."""
    import torch
    R, fl, x = (torch.tensor(a.astype(np.float64)) for a in (R, fl, jar))
    x.requires_grad_(True)
    T = torch.tensor(T)
    rf = R * fl
    quad = 0.5 * x * x / R
    lin = fl * (torch.abs(x) - 0.5 * rf)
    s = torch.where(T == TR_EQUALITY, quad, torch.where(T == TR_FRICTION, torch.where(torch.abs(x) >= rf, lin, quad),
                                                        torch.where(x < 0, quad, torch.zeros_like(x))))
    g, = torch.autograd.grad(s.sum(), x, create_graph=True)
    h, = torch.autograd.grad(g.sum(), x)
    scale = torch.where((T == TR_FRICTION) & (torch.abs(x) >= rf), fl * (torch.abs(x) + 0.5 * rf), s)
    return s.detach().numpy(), -g.detach().numpy(), h.numpy(), scale.detach().numpy()


def check_rows(kind, engine):
    T, R, fl, jar = row_cases()
    if engine == "so100":              # (no equality rows in the SO100 engine; a row is a friction row when floss > 0)
        keep = T != TR_EQUALITY
        T, R, fl, jar = T[keep], R[keep], fl[keep], jar[keep]
        out = probes(kind).so100_row(R, fl, jar)
    else:
        out = probes(kind).tree_scalar(T, (1.0 / R.astype(np.float64)).astype(F), R, fl, jar)
    assert np.all(np.isfinite(out))
    cost, force, h, scale = row_reference(T, R, fl, jar)
    lin = (T == TR_FRICTION) & (np.abs(jar.astype(np.float64)) >= R.astype(np.float64) * fl)
    assert lin.sum() >= 100 and (~lin & (T == TR_FRICTION)).sum() >= 100
    # piecewise-linear parts and inactive rows: exact force and curvature
    np.testing.assert_array_equal(out[lin, 1], force[lin].astype(F))
    assert not np.any(out[lin, 2])
    assert not np.any(out[(T == TR_LIMIT) & (jar >= 0)])
    tiny = np.finfo(np.float64).tiny
    ec = np.abs(out[:, 0] - cost) / np.maximum(scale, tiny)
    ef = np.abs(out[:, 1] - force) / np.maximum(np.abs(force), tiny)
    eh = np.abs(out[:, 2] - h) / np.maximum(np.abs(h), tiny)
    for name, e in (("cost", ec), ("force", ef), ("h", eh)):
        assert worst(f"{kind} {engine} row {name}", float(e.max()), ROW_REL) <= ROW_REL, int(np.argmax(e))


# ============================================================================================ B. wave primitives: the model
LANES = np.arange(64)
_X1, _X2 = LANES ^ 1, LANES ^ 2
_HM, _RM = (LANES & ~7) | (7 - (LANES & 7)), (LANES & ~15) | (15 - (LANES & 15))


def model_row_sums(v):
    """(ncase, 64) float32: what every lane holds after the four butterfly steps inside its row of 16"""
    t = np.asarray(v, F)
    for perm in (_X1, _X2, _HM, _RM):
        t = (t + t[:, perm]).astype(F)
    return t


def model_sum(v):
    t = model_row_sums(v)
    return ((t[:, 0] + t[:, 16]).astype(F) + (t[:, 32] + t[:, 48]).astype(F)).astype(F)


def model_sum_row0(v):
    return (model_row_sums(v)[:, 0] + F(0)).astype(F)


def model_argmax(val, idx, payload=None, groups=1, by_candidate=True):
    """largest value, smallest index on ties, payload of the lowest such lane; per group of 64 / groups lanes.  Returns per-lane arrays.
    As wave.hpp specifies it: a lane's candidate is its index where it holds the maximum and 0x7fffffff otherwise, the payload comes from the
    lowest lane whose candidate equals the smallest one - so when the winning index IS 0x7fffffff (the index of a lane without an entry) that
    may be a lane which does not hold the maximum.  by_candidate=False: the row butterflies (row_argmax3), which carry the winning lane's
    own payload whatever its index."""
    val, idx = np.asarray(val, F), np.asarray(idx, np.int32)
    n, w = len(val), 64 // groups
    ov, oi, src = np.empty_like(val), np.empty_like(idx), np.empty((n, 64), int)
    for g in range(groups):
        s = slice(g * w, (g + 1) * w)
        m = val[:, s].max(axis=1)
        cand = np.where(val[:, s] == m[:, None], idx[:, s].astype(np.int64), 0x7fffffff)
        best = cand.min(axis=1)
        ov[:, s], oi[:, s] = m[:, None], best[:, None]
        hit = (cand == best[:, None]) if by_candidate else ((val[:, s] == m[:, None]) & (idx[:, s] == best[:, None]))
        src[:, s] = (g * w + np.argmax(hit, axis=1))[:, None]
    if payload is None:
        return ov, oi
    return ov, oi, np.take_along_axis(np.asarray(payload, F), src[:, None, :].repeat(payload.shape[1], axis=1), axis=2)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _sum_inputs():
    rng = np.random.RandomState(5)
    n = 256
    v = (rng.normal(size=(n, 64)) * _loguniform(rng, 1e-30, 1e8, (n, 64))).astype(F)
    v[32:64] = (rng.randint(-2 ** 22, 2 ** 22, size=(32, 64)) * np.float64(2.0 ** -149)).astype(F)        # subnormal addends
    v[64:96, 32:] = -v[64:96, :32]                                                                         # exact cancellations across rows
    v[96:128, 1::2] = -v[96:128, 0::2]                                                                     # ... and between neighbours
    v[128:144] = F(-0.0)
    v[144:160] = F(0.0)
    v[160:176] = np.where(rng.rand(16, 64) < 0.5, F(-0.0), F(0.0))
    v[176:192] = (rng.normal(size=(16, 64)) * 1e-40).astype(F) + F(1e8) * (rng.rand(16, 64) < 0.05)
    return v


def _row0_inputs():
    v = _sum_inputs()
    v[:, 16:] = F(0.0)
    v[128:144, :16] = F(-0.0)            # row 0 sums to -0.0
    return v


def check_wave_sums(kind):
    P = probes(kind)
    v = _sum_inputs()
    want = np.repeat(model_sum(v)[:, None], 64, axis=1)
    for op in ("sum", "sum_rows"):
        got = P.wave(op, v[:, None, :])[0][:, 0]
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=op)
    v0 = _row0_inputs()
    full = P.wave("sum", v0[:, None, :])[0][:, 0]
    short = P.wave("sum_row0", v0[:, None, :])[0][:, 0]
    np.testing.assert_array_equal(_bits(short), _bits(full))
    np.testing.assert_array_equal(_bits(short), _bits(np.repeat(model_sum_row0(v0)[:, None], 64, axis=1)))
    np.testing.assert_array_equal(_bits(full), _bits(np.repeat(model_sum(v0)[:, None], 64, axis=1)))
    assert np.all(_bits(full[128:144]) == 0)          # (-0.0) + (+0.0) = +0.0


def _argmax_inputs():
    """val (n, 64), idx (n, 64), payload (n, 3, 64)"""
    rng = np.random.RandomState(6)
    n = 256
    val = rng.normal(size=(n, 64)).astype(F)
    idx = np.stack([rng.permutation(64) for _ in range(n)]).astype(np.int32) * 7 + 3
    for k in range(64):                  # the maximum in every lane in turn
        val[k, k] = F(10.0)
    val[64:80] = F(1.5)                  # all equal
    for k in range(80, 112):             # ties across rows: the maximum twice or more, in different rows
        val[k, rng.choice(64, size=rng.randint(2, 6), replace=False)] = F(7.0)
    for k in range(112, 144):            # duplicated indices on tied lanes: the payload is that of the lowest such lane
        lanes = rng.choice(64, size=rng.randint(2, 8), replace=False)
        val[k, lanes] = F(7.0)
        idx[k, lanes] = 1
    idx[144:160, :] = 0x7fffffff         # index 0x7fffffff everywhere ...
    idx[160:176, ::3] = 0x7fffffff       # ... and among others
    val[176:192] = np.where(rng.rand(16, 64) < 0.5, F(-0.0), F(0.0))       # mixed-sign zeros (values compare with ==)
    val[192:208] = (rng.normal(size=(16, 64)) * _loguniform(rng, 1e-30, 1e8, (16, 64))).astype(F)
    val[208:224] = -np.abs(val[208:224])
    idx[224:240, 5::16] = 0x7fffffff     # ... one per row
    pay = rng.normal(size=(n, 3, 64)).astype(F)
    return val, idx, pay


def check_wave_extrema(kind):
    P = probes(kind)
    val, idx, pay = _argmax_inputs()
    n = len(val)
    m = val.max(axis=1)
    got = P.wave("max", val[:, None, :])[0][:, 0]
    assert np.all(got == m[:, None])
    got = P.wave("min_i", None, idx[:, None, :], ncase=n)[1][:, 0]
    np.testing.assert_array_equal(got, np.repeat(idx.min(axis=1)[:, None], 64, axis=1))
    signed = (idx * np.where(val < 0, -1, 1)).astype(np.int32)
    got = P.wave("min_i", None, signed[:, None, :], ncase=n)[1][:, 0]
    np.testing.assert_array_equal(got, np.repeat(signed.min(axis=1)[:, None], 64, axis=1))
    wv, wi, wp = model_argmax(val, idx, pay)
    fo, io = P.wave("argmax", val[:, None, :], idx[:, None, :])
    assert np.all(fo[:, 0] == wv)
    np.testing.assert_array_equal(io[:, 0], wi)
    fo, io = P.wave("argmax3", np.concatenate([val[:, None, :], pay], axis=1), idx[:, None, :])
    assert np.all(fo[:, 0] == wv)
    np.testing.assert_array_equal(io[:, 0], wi)
    assert np.sum(wi[:, 0] == 0x7fffffff) >= 16          # (the sentinel wins: the payload is the one wave.hpp documents for that case)
    np.testing.assert_array_equal(_bits(fo[:, 1:4]), _bits(wp))


def check_wave_rows(kind):
    """row_argmax3 / row_argmax with each of the 15 non-empty subsets of rows active and the others branched out; whole rows, distinct
    indices inside a row (the contract of wave.hpp)"""
    P = probes(kind)
    val, idx, pay = _argmax_inputs()
    keep = np.r_[0:112, 176:256]          # (not the duplicated-index and the all-0x7fffffff cases: indices are distinct inside a row)
    val, idx, pay = val[keep], idx[keep], pay[keep]
    keep = np.array([all(len(set(r[16 * g:16 * g + 16])) == 16 for g in range(4)) for r in idx])
    val, idx, pay = val[keep], idx[keep], pay[keep]
    n = len(val)
    assert n >= 150
    wv, wi, wp = model_argmax(val, idx, pay, groups=4, by_candidate=False)
    subsets = np.arange(n) % 15 + 1
    act = ((subsets[:, None] >> (LANES[None, :] >> 4)) & 1).astype(np.int32)
    for s in range(1, 16):
        assert np.sum(subsets == s) >= 8
    ii = np.stack([idx, act], axis=1)
    fo, io = P.wave("row_argmax3", np.concatenate([val[:, None, :], pay], axis=1), ii)
    on = act.astype(bool)
    assert np.all(fo[:, 0][on] == wv[on])
    np.testing.assert_array_equal(io[:, 0][on], wi[on])
    on3 = np.repeat(on[:, None, :], 3, axis=1)
    np.testing.assert_array_equal(_bits(fo[:, 1:4])[on3], _bits(wp)[on3])
    assert not np.any(fo[:, 0][~on]) and not np.any(io[:, 0][~on]) and not np.any(_bits(fo[:, 1:4])[~on3])
    fo, io = P.wave("row_argmax", val[:, None, :], ii)
    assert np.all(fo[:, 0][on] == wv[on])
    np.testing.assert_array_equal(io[:, 0][on], wi[on])
    assert not np.any(fo[:, 0][~on]) and not np.any(io[:, 0][~on])


def check_wave_moves(kind):
    """ballot + prefix, wave_get_*, wave_bcast_*, wave_xor32_f"""
    P = probes(kind)
    rng = np.random.RandomState(8)
    n = 256
    pred = (rng.rand(n, 64) < rng.rand(n, 1)).astype(np.int32)
    pred[0], pred[1] = 0, 1
    pred[2:66] = np.eye(64, dtype=np.int32)
    io = P.wave("ballot", None, pred[:, None, :] * rng.randint(1, 1 << 30, size=(n, 1, 64)), ncase=n)[1]
    np.testing.assert_array_equal(io[:, 0], np.cumsum(pred, axis=1) - pred)
    mask = np.sum(pred.astype(np.uint64) << LANES.astype(np.uint64)[None, :], axis=1, dtype=np.uint64)
    np.testing.assert_array_equal(io[:, 1].view(np.uint32), np.repeat((mask & np.uint64(0xffffffff)).astype(np.uint32)[:, None], 64, axis=1))
    np.testing.assert_array_equal(io[:, 2].view(np.uint32), np.repeat((mask >> np.uint64(32)).astype(np.uint32)[:, None], 64, axis=1))
    v = (rng.normal(size=(n, 64)) * _loguniform(rng, 1e-30, 1e8, (n, 64))).astype(F)
    w = rng.randint(-2 ** 31, 2 ** 31, size=(n, 64)).astype(np.int32)
    src = np.repeat((np.arange(n) % 64)[:, None], 64, axis=1).astype(np.int32)
    fo, io = P.wave("get", v[:, None, :], np.stack([w, src], axis=1))
    np.testing.assert_array_equal(_bits(fo[:, 0]), _bits(np.take_along_axis(v, src, axis=1)))
    np.testing.assert_array_equal(io[:, 0], np.take_along_axis(w, src, axis=1))
    src = rng.randint(0, 64, size=(n, 64)).astype(np.int32)
    src[:64] = np.repeat(np.arange(64)[:, None], 64, axis=1)
    fo, io = P.wave("bcast", v[:, None, :], np.stack([w, src], axis=1))
    np.testing.assert_array_equal(_bits(fo[:, 0]), _bits(np.take_along_axis(v, src, axis=1)))
    np.testing.assert_array_equal(io[:, 0], np.take_along_axis(w, src, axis=1))
    fo, _ = P.wave("xor32", v[:, None, :])
    np.testing.assert_array_equal(_bits(fo[:, 0]), _bits(v[:, LANES ^ 32]))


def mfma_unpack(acc):
    """(ncase, 64, 16) accumulators -> (ncase, 32, 32) matrices, by the layout documented in wave.hpp"""
    D = np.empty((len(acc), 32, 32), acc.dtype)
    for l in range(64):
        for r in range(16):
            D[:, 8 * (r // 4) + 4 * (l // 32) + r % 4, l % 32] = acc[:, l, r]
    return D


def mfma_operands(a, b):
    """per-lane operands (ncase, ncall, 64) -> A (ncase, ncall, 32, 2), B (ncase, ncall, 2, 32): lane l supplies A[l % 32][l / 32], B[l / 32][l % 32]"""
    A = np.stack([a[:, :, :32], a[:, :, 32:]], axis=3)
    B = np.stack([b[:, :, :32], b[:, :, 32:]], axis=2)
    return A, B


def check_mfma(kind):
    P = probes(kind)
    rng = np.random.RandomState(9)
    # small integers: every product and sum is exact, so the layout alone decides (|v| <= 64, up to 18 calls: sums below 2^24)
    for ncall in (1, 3, MFMA_CALLS):
        a = rng.randint(-64, 65, size=(32, ncall, 64)).astype(F)
        b = rng.randint(-64, 65, size=(32, ncall, 64)).astype(F)
        A, B = mfma_operands(a.astype(np.int64), b.astype(np.int64))
        want = np.einsum("ncik,nckj->nij", A, B)
        assert np.abs(want).max() < 2 ** 24
        np.testing.assert_array_equal(mfma_unpack(P.mfma(a, b)).astype(np.int64), want)
    a = (rng.normal(size=(64, MFMA_CALLS, 64)) * _loguniform(rng, 1e-3, 1e3, (64, MFMA_CALLS, 64))).astype(F)
    b = (rng.normal(size=(64, MFMA_CALLS, 64)) * _loguniform(rng, 1e-3, 1e3, (64, MFMA_CALLS, 64))).astype(F)
    A, B = mfma_operands(a.astype(np.float64), b.astype(np.float64))
    want, mag = np.einsum("ncik,nckj->nij", A, B), np.einsum("ncik,nckj->nij", np.abs(A), np.abs(B))
    e = np.abs(mfma_unpack(P.mfma(a, b)) - want) / mag
    assert worst(f"{kind} mfma 18 calls / sum |a||b|", float(e.max()), MFMA_GAMMA) <= MFMA_GAMMA


# ============================================================================================ C. small math
@functools.lru_cache(maxsize=None)
def sincos_inputs():
    rng = np.random.RandomState(11)
    k = np.arange(-6366, 6367)
    near = (k * (np.pi / 2)).astype(F)
    nb = [near]
    lo, hi = near.copy(), near.copy()
    for _ in range(8):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        nb += [lo, hi]
    x = np.concatenate([rng.uniform(-1e4, 1e4, 400000).astype(F), rng.uniform(-np.pi, np.pi, 300000).astype(F), np.concatenate(nb),
                        (rng.uniform(-1, 1, 60000) * 1e-3).astype(F), (rng.normal(size=40000) * _loguniform(rng, 1e-30, 1e-3, 40000)).astype(F),
                        np.array([0.0, -0.0], F)])
    x = x[np.abs(x) < 1e4]
    x.setflags(write=False)
    return x


def ulp_error(got, want64):
    """|got - want| in units of the float32 spacing at the correctly rounded result"""
    return np.abs(got.astype(np.float64) - want64) / np.spacing(np.abs(want64.astype(F))).astype(np.float64)


def check_sincos(kind):
    P = probes(kind)
    x = sincos_inputs()
    assert 1000000 <= len(x) <= 1100000
    s, c = np.empty_like(x), np.empty_like(x)
    for a in range(0, len(x), 1 << 19):
        s[a:a + (1 << 19)], c[a:a + (1 << 19)] = P.sincos(x[a:a + (1 << 19)])
    x64 = x.astype(np.float64)
    es, ec = ulp_error(s, np.sin(x64)), ulp_error(c, np.cos(x64))
    ws, wc = worst(f"{kind} sincos_f sin, ulp", float(es.max()), SINCOS_ULP), worst(f"{kind} sincos_f cos, ulp", float(ec.max()), SINCOS_ULP)
    z = x == 0
    assert z.sum() >= 2
    np.testing.assert_array_equal(_bits(s[z]), _bits(x[z]))              # sin(+-0) = +-0, sign and all
    assert np.all(c[z] == 1.0)
    assert ws <= SINCOS_ULP and wc <= SINCOS_ULP, (float(x[np.argmax(es)]), float(x[np.argmax(ec)]))


def q2m64(q):
    w, x, y, z = (q[..., i] for i in range(4))
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1).reshape(q.shape[:-1] + (3, 3))


def qmul64(p, q):
    return np.stack([p[..., 0] * q[..., 0] - p[..., 1] * q[..., 1] - p[..., 2] * q[..., 2] - p[..., 3] * q[..., 3],
                     p[..., 0] * q[..., 1] + p[..., 1] * q[..., 0] + p[..., 2] * q[..., 3] - p[..., 3] * q[..., 2],
                     p[..., 0] * q[..., 2] - p[..., 1] * q[..., 3] + p[..., 2] * q[..., 0] + p[..., 3] * q[..., 1],
                     p[..., 0] * q[..., 3] + p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1] + p[..., 3] * q[..., 0]], axis=-1)


def mat2quat_branch(m):
    """the branch mat2quat takes, from the float32 matrix in float32 arithmetic (sums only: exact restatement)"""
    m = np.asarray(m, F).reshape(-1, 9)
    t = ((m[:, 0] + m[:, 4]).astype(F) + m[:, 8]).astype(F)
    return np.where(t > 0, 0, np.where((m[:, 0] > m[:, 4]) & (m[:, 0] > m[:, 8]), 1, np.where(m[:, 4] > m[:, 8], 2, 3)))


@functools.lru_cache(maxsize=None)
def quat_cases():
    """float32 inputs of the quaternion probe: qa, qb (unit up to rounding), s6, R = quat2mat(qa) in float64 rounded, m = rotation matrices
    that reach the four branches of mat2quat, and the float64 quaternion each m was made from"""
    rng = np.random.RandomState(12)
    n = 2400

    def unit(a):
        return a / np.linalg.norm(a, axis=1, keepdims=True)
    qa, qb = unit(rng.normal(size=(n, 4))), unit(rng.normal(size=(n, 4)))
    s6 = rng.normal(size=(n, 6)) * _loguniform(rng, 1e-3, 1e3, (n, 1))
    qm = unit(rng.normal(size=(n, 4)))
    axes = np.concatenate([np.eye(3)[np.arange(240) % 3] + 0.05 * rng.normal(size=(240, 3)), rng.normal(size=(160, 3)),
                           np.tile(np.array([[1.0, 1.0, 1.0], [1.0, -1.0, 1.0]]), (20, 1))])
    ang = np.pi - 1e-3
    qm[:len(axes)] = np.concatenate([np.full((len(axes), 1), np.cos(ang / 2)), np.sin(ang / 2) * unit(axes)], axis=1)
    qa32, qb32 = qa.astype(F), qb.astype(F)
    res = dict(qa=qa32, qb=qb32, s6=s6.astype(F), R=q2m64(qa32.astype(np.float64)).astype(F), m=q2m64(qm).astype(F), qm=qm)
    for v in res.values():
        v.setflags(write=False)
    return res


def quat_reference(c):
    """float64 results from the float32 inputs: dict like Probes.quat()"""
    qa, qb, s6, R = (c[k].astype(np.float64) for k in ("qa", "qb", "s6", "R"))
    S = np.stack([s6[:, 0], s6[:, 3], s6[:, 4], s6[:, 3], s6[:, 1], s6[:, 5], s6[:, 4], s6[:, 5], s6[:, 2]], axis=1).reshape(-1, 3, 3)
    RS = R @ S @ R.transpose(0, 2, 1)
    v = qb[:, :3]
    nv = np.linalg.norm(v, axis=1)
    return dict(quat2mat=q2m64(qa), mulquat=qmul64(qa, qb), normquat=qa / np.linalg.norm(qa, axis=1, keepdims=True),
                normalize3=v / nv[:, None], norm3=nv,
                rotsym=np.stack([RS[:, 0, 0], RS[:, 1, 1], RS[:, 2, 2], RS[:, 0, 1], RS[:, 0, 2], RS[:, 1, 2]], axis=1),
                mat2quat=c["qm"], rotvecquat=np.einsum("nij,nj->ni", q2m64(qa), qb[:, 1:]))


def quat_errors(got, c):
    ref = quat_reference(c)
    mx = lambda a: np.abs(a).reshape(len(a), -1).max(axis=1)                 # noqa: E731
    e = {k: mx(got[k] - ref[k]) for k in ("quat2mat", "mulquat", "normquat")}
    e["normalize3"] = np.maximum(mx(got["normalize3"] - ref["normalize3"]), np.abs(got["norm3"] - ref["norm3"]) / ref["norm3"])
    e["rotsym"] = mx(got["rotsym"] - ref["rotsym"]) / mx(c["s6"])
    e["mat2quat"] = np.minimum(mx(got["mat2quat"] - ref["mat2quat"]), mx(got["mat2quat"] + ref["mat2quat"]))
    e["rotvecquat"] = mx(got["rotvecquat"] - ref["rotvecquat"]) / np.linalg.norm(c["qb"][:, 1:].astype(np.float64), axis=1)
    return e


QUAT_BOUNDS = {"quat2mat": "QUAT2MAT", "mulquat": "MULQUAT", "normquat": "NORMQUAT", "normalize3": "NORMALIZE3", "rotsym": "ROTSYM",
               "mat2quat": "MAT2QUAT", "rotvecquat": "ROTVECQUAT"}


def check_quat(kind):
    P = probes(kind)
    c = quat_cases()
    br = mat2quat_branch(c["m"])
    assert all(np.sum(br == b) >= 50 for b in range(4)), np.bincount(br)
    got = P.quat(c["qa"], c["qb"], c["s6"], c["R"], c["m"])
    for k, v in got.items():
        assert np.all(np.isfinite(v)), k
    e = quat_errors(got, c)
    bad = []
    for k, name in QUAT_BOUNDS.items():
        b = globals()[name]
        if not worst(f"{kind} {k}", float(e[k].max()), b) <= b:
            bad.append((k, float(e[k].max()), int(np.argmax(e[k]))))
    for b in range(4):
        worst(f"{kind} mat2quat branch {b}", float(e["mat2quat"][br == b].max()), MAT2QUAT)
    assert not bad, bad
    # below MINVAL_F: the documented fallbacks (1, 0, 0) with return value 0, and the identity quaternion
    n = 64
    tiny = np.zeros((n, 4), F)
    tiny[1:] = (np.random.RandomState(13).normal(size=(n - 1, 4)) * 1e-17).astype(F)
    z = np.zeros((n, 9), F)
    got = P.quat(tiny, tiny, np.zeros((n, 6), F), z, z)
    np.testing.assert_array_equal(got["normquat"], np.tile(np.array([1, 0, 0, 0], F), (n, 1)))
    np.testing.assert_array_equal(got["normalize3"], np.tile(np.array([1, 0, 0], F), (n, 1)))
    assert not np.any(got["norm3"])


@functools.lru_cache(maxsize=None)
def impedance_cases():
    """solimp (n, 5), pos (n,) float32.  Widths are powers of two wherever x = |pos| / width has to come out exactly."""
    rng = np.random.RandomState(14)
    rows, pos = [], []
    for c in range(3000):
        power = (1.0, 2.0, 3.0)[c % 3]
        dmin, dmax = sorted(rng.uniform(0.0, 1.0, 2))
        mid = rng.randint(1, 16) / 16.0
        width = 2.0 ** rng.randint(-8, 1)
        k = (c // 3) % 10
        x = [0.0, mid, 1.0, rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0, mid), rng.uniform(mid, 1), rng.uniform(1, 3), mid * (1 - 2.0 ** -12), mid * (1 + 2.0 ** -12)][k]
        if c % 50 == 7:
            width = 0.0
        if c % 50 == 11:
            dmax = dmin
        if c % 50 == 13:
            dmin, dmax = -0.5, 1.5                  # outside [1e-4, 0.9999]: clamped
        if c % 50 == 17:
            dmin, dmax = 5e-5, 0.99995
        if c % 50 == 19:
            mid = (0.0, 1.0)[(c // 50) % 2]                # clamped as well
        if c % 50 == 23:
            width = rng.uniform(1e-3, 1.0)          # a width that is no power of two
        rows.append([dmin, dmax, width, mid, power])
        pos.append(x * width * (1 if c % 2 else -1))
    a, p = np.array(rows, F), np.array(pos, F)
    a.setflags(write=False), p.setflags(write=False)
    return a, p


def impedance_reference(solimp, pos):
    """float64, the generic formula x^p / mid^(p - 1) for every power (so101_math.hpp's power-2 closed form must agree with it at p = 2)"""
    s, pos = solimp.astype(np.float64), pos.astype(np.float64)
    lo, hi = np.float64(F(MINIMP)), np.float64(F(MAXIMP))
    dmin, dmax, mid = np.clip(s[:, 0], lo, hi), np.clip(s[:, 1], lo, hi), np.clip(s[:, 3], lo, hi)
    width, p = np.maximum(s[:, 2], 0.0), np.maximum(s[:, 4], 1.0)
    flat = (dmin == dmax) | (width <= np.float64(F(MINVAL)))
    with np.errstate(all="ignore"):
        x = np.abs(pos) / np.where(flat, 1.0, width)
        xc = np.clip(x, 0.0, 1.0)
        y = np.where(xc <= mid, xc ** p / mid ** (p - 1), 1 - (1 - xc) ** p / (1 - mid) ** (p - 1))
        y = np.where(p == 1.0, xc, y)
    return np.where(flat, 0.5 * (dmin + dmax), np.where(x >= 1, dmax, np.where(x <= 0, dmin, dmin + y * (dmax - dmin))))


def check_impedance(kind):
    solimp, pos = impedance_cases()
    got = probes(kind).impedance(solimp, pos)
    ref = impedance_reference(solimp, pos)
    e = np.abs(got - ref)
    for p in (1.0, 2.0, 3.0):
        worst(f"{kind} impedance power {p:g}", float(e[solimp[:, 4] == p].max()), IMPEDANCE)
    assert e.max() <= IMPEDANCE, int(np.argmax(e))
    # x exactly 0 and >= 1: the end values, exactly
    x = np.abs(pos.astype(np.float64)) / np.maximum(solimp[:, 2].astype(np.float64), 1e-300)
    flat = (np.clip(solimp[:, 0], F(MINIMP), F(MAXIMP)) == np.clip(solimp[:, 1], F(MINIMP), F(MAXIMP))) | (solimp[:, 2] <= F(MINVAL))
    ends = ~flat & ((x <= 0) | (x >= 1)) & (np.frexp(solimp[:, 2])[0] == 0.5)          # (powers of two: x comes out exactly)
    assert ends.sum() >= 300
    np.testing.assert_array_equal(got[ends], ref[ends].astype(F))


M32 = 0xFFFFFFFF


def philox_uniform(seed, env, episode, draw):
    """Philox4x32-10 in Python integers, from the published round function; the first output word's top 24 bits as a float in [0, 1)"""
    c0, c1, c2, c3 = env & M32, (env >> 32) & M32, episode & M32, draw & M32
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return (c0 >> 8) / 16777216.0


def check_rng(kind):
    # the round function against the known-answer vectors of the Random123 distribution (counter, key -> first output word)
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), 0x6627e8d5), ((M32, M32, M32, M32), (M32, M32), 0x408f276d),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 0xd16cfe09)):
        u = philox_uniform(key[0] | key[1] << 32, ctr[0] | ctr[1] << 32, ctr[2], ctr[3])
        assert u == (want >> 8) / 16777216.0, hex(want)
    rng = np.random.RandomState(15)
    n = 4096
    big = lambda: [int(rng.randint(0, 1 << 32)) | int(rng.randint(0, 1 << 32)) << 32 for _ in range(n)]         # noqa: E731
    seed, env = big(), big()
    for k in range(0, n, 4):
        seed[k] &= M32                            # small seeds and env ids, as the scenes use them ...
        env[k] = k // 4
    seed[1], env[1], seed[2], env[2] = (1 << 64) - 1, (1 << 64) - 1, 1 << 32, 1 << 32      # ... and the ends of the range
    edge = [0, M32, 1, 0x80000000]
    ep = [edge[k % 4] if k % 3 == 0 else int(rng.randint(0, 1 << 32)) for k in range(n)]
    draw = [edge[(k // 4) % 4] if k % 3 == 1 else int(rng.randint(0, 1 << 32)) for k in range(n)]
    got = probes(kind).rng(np.array(seed, np.uint64), np.array(env, np.uint64), np.array(ep, np.uint32), np.array(draw, np.uint32))
    want = np.array([philox_uniform(*t) for t in zip(seed, env, ep, draw)])
    np.testing.assert_array_equal(got.astype(np.float64), want)
    assert np.all((got >= 0) & (got < 1))
    assert 0.45 < got.mean() < 0.55


def check_tri(kind):
    t = probes(kind).tri(18)
    i, j = np.meshgrid(np.arange(18), np.arange(18), indexing="ij")
    hi, lo = np.maximum(i, j), np.minimum(i, j)
    np.testing.assert_array_equal(t, hi * (hi + 1) // 2 + lo)
    assert sorted(t[np.tril_indices(18)]) == list(range(171))          # the packed lower triangle, each slot once
