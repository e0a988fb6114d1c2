"""Shared cases of the solute-transport tests (test_transport_twin.py, test_gpu_transport.py): levels of hexahedra, triangles,
quadrilaterals and agglomerated elements with their pore volumes, four lognormal permeability fields each, the oracle's
direct-solve fluxes on them plus a fifth column of zero flux, and the cached twin results.  No tests here.

    case             source                                        elements   row entries
    hex0, hex1       tracer_cases.hierarchy("hex") levels 0 / 1    512 / 64   6
    stretch          tracer_cases, 4 x 3 x 5                       60         6
    tri1             derivative_family_cases "tri" level 1         328        3
    quad0, quad1     "quad" levels 0 / 1                           60 / 15    4
    agg2_1, agg2_2   "agg2" levels 1 / 2                           41 / 5     5-12 / 6-10
    agg3_1           "agg3" level 1                                334        4-15

The derivative-family problems carry nonzero essential fluxes: inflow through "closed" sides.  The results are cached: the
tests read them and leave them unchanged."""
import dataclasses
import functools

import numpy as np

import derivative_family_cases as dfc
import tracer_cases as trc
from parelagmc_amd.fe import transport as tw

SOURCES = {"hex0": ("hex", 0), "hex1": ("hex", 1), "stretch": ("stretch", 0), "tri1": ("tri", 1), "quad0": ("quad", 0),
           "quad1": ("quad", 1), "agg2_1": ("agg2", 1), "agg2_2": ("agg2", 2), "agg3_1": ("agg3", 1)}
NAMES = tuple(SOURCES)
POROSITY = 0.3
CFL = 0.9
NREPORT = 16                 # on quad1 and agg2_2 more than the step count: several reports fall into one step
MARGIN = 1e-9                # columns whose ceil() margin is below this are left out of twin / kernel comparisons ...
MARGIN_E = 1e-6              # ... and of the end-to-end comparison below this; at most one column of a case either way


def problem(kind):
    return trc.problem(kind) if kind in ("hex", "stretch") else dfc.problem(kind)


@functools.lru_cache(maxsize=None)
def volumes(kind, level):
    """element volumes of a level; on agglomerated levels the finest volumes restricted with the levels' P^T"""
    if kind in ("hex", "stretch"):
        return trc.hierarchy(kind).spaces[level].vol.copy()
    if kind in ("tri", "quad"):
        return dfc.hierarchy(kind).spaces[level].vol.copy()
    v = dfc.tet_spaces(int(kind[3])).vol.copy()
    for L in problem(kind).levels[:level]:
        v = np.asarray(L.P.T @ v).ravel()
    return v


def smoothed_lognormal(B, sigma, rng, passes=3):
    """exp(sigma g): g white noise averaged `passes` times over the face neighbours, scaled to unit variance"""
    A = (abs(B) @ abs(B).T).tocsr()
    A = A.multiply(1.0 / A.sum(axis=1)).tocsr()
    g = rng.standard_normal(B.shape[0])
    for _ in range(passes):
        g = A @ g
    g = (g - g.mean()) / g.std()
    return np.exp(sigma * g)


@dataclasses.dataclass
class Case:
    name: str
    kind: str
    level: int
    dlevel: object            # the DarcyLevel
    mesh: tw.TransportMesh
    k: np.ndarray             # (4, n_p): sigma 1, 1, 2, 2
    u: np.ndarray             # (5, n_u): the oracle's fluxes on k, and a column of zero flux
    t_end: float              # total pore volume over the median boundary inflow rate of the four fields


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    from oracle.darcy_oracle import DarcyOracle
    kind, level = SOURCES[name]
    dp = problem(kind)
    L = dp.levels[level]
    mesh = tw.transport_mesh(L, volumes(kind, level), POROSITY)
    rng = np.random.Generator(np.random.PCG64(20261020 + NAMES.index(name)))
    k = np.stack([smoothed_lognormal(L.B, s, rng) for s in (1.0, 1.0, 2.0, 2.0)])
    orc = DarcyOracle(dp)
    u = np.stack([orc.solve_fwd(level, kk, True)[2][:L.n_u] for kk in k] + [np.zeros(L.n_u)])
    t_end = float(mesh.pore_volume.sum() / np.median(tw.inflow_mass_rate(mesh, u[:4])))
    for a in (k, u):
        a.setflags(write=False)
    return Case(name, kind, level, L, mesh, k, u, t_end)


@functools.lru_cache(maxsize=None)
def twin(name, nreport=NREPORT, longdouble=False):
    """the twin on the case's five columns"""
    c = case(name)
    return tw.advance(c.mesh, c.u, c.t_end, CFL, nreport, dtype=np.longdouble if longdouble else np.float64)


def kept(margin, threshold=MARGIN):
    """columns a comparison keeps.  Asserts that at most one is left out."""
    keep = np.asarray(margin) >= threshold
    assert (~keep).sum() <= 1, f"{(~keep).sum()} columns have a decision margin below {threshold}"
    return keep


def injected(mesh, u, t_reached):
    """the solute mass that entered by t_reached, per column"""
    return np.asarray(t_reached, np.float64) * tw.inflow_mass_rate(mesh, u).astype(np.float64)


def deviation(mesh, u, got, ref, keep):
    """largest difference of two results over the kept columns: c absolutely, curve and stored relative to the injected mass
    (columns into which nothing was injected must agree exactly)"""
    inj = injected(mesh, u, ref["t_reached"])
    worst = 0.0
    for b in np.flatnonzero(keep):
        dc = float(np.abs(got["c"][b] - ref["c"][b]).max())
        dm = max(float(np.abs(got["curve"][b] - ref["curve"][b]).max()), float(abs(got["stored"][b] - ref["stored"][b])))
        if inj[b] > 0:
            dm /= inj[b]
        else:
            assert dm == 0.0
        worst = max(worst, dc, dm)
    return worst


# ---- measured tolerances (re-measured by test_transport_twin.py::test_recorded_tolerances) ----------
# Largest deviation of the float64 twin from the np.longdouble twin over all cases and kept columns, nreport 16: c absolutely,
# curve and stored relative to the injected mass.  The kernel may differ from the twin by 16 x that: the factor covers the
# device's divisions and the order of the reductions.  Measured: 4.2e-15 (hex0, its column of 281 steps).
ROUNDING_RAW = 5.0e-15
TOL_K = 16 * ROUNDING_RAW
# Largest change of the twin's results, measured the same way, when every flux is multiplied by 1 + 1e-8 N(0, 1) (three
# draws) - the agreement test_gpu_parity.py demands of a 1e-12 solve against the oracle.  A 1e-12 solve may differ from the
# twin on the oracle's flux by 10 x that.  Measured: 7.7e-8 (hex0).
PERTURBATION_RAW = 9.0e-8
TOL_E = 10 * PERTURBATION_RAW


def rounding_deviation(name):
    c, r, rl = case(name), twin(name), twin(name, longdouble=True)
    keep = kept(r["margin"])
    assert (r["nsteps"] == rl["nsteps"])[keep].all() and (r["status"] == rl["status"])[keep].all()
    return deviation(c.mesh, c.u, r, rl, keep)


def perturbation_change(name, reps=3, size=1e-8):
    c, r = case(name), twin(name)
    keep = kept(r["margin"])
    rng = np.random.Generator(np.random.PCG64(7))
    worst = 0.0
    for _ in range(reps):
        rp = tw.advance(c.mesh, c.u * (1 + size * rng.standard_normal(c.u.shape)), c.t_end, CFL, NREPORT)
        k2 = keep & (rp["nsteps"] == r["nsteps"])
        assert (~k2).sum() <= 1
        worst = max(worst, deviation(c.mesh, c.u, rp, r, k2))
    return worst


# ---- what create refuses ----------------------------------------------------------------------------------------------
def bad_meshes(mesh):
    """(label, mesh) for every refusal of pmc_transport_create that concerns the mesh; for the twin's validate and for the device"""
    ne, nf = mesh.n_elem, mesh.n_face
    s = tw.validate(mesh)
    interior = int(np.flatnonzero(~s.boundary)[0])
    pos = np.flatnonzero(mesh.col == interior)

    def changed(**kw):
        return dataclasses.replace(mesh, **kw)

    def with_entry(name, index, value, dtype=None):
        default = s.boundary if name == "outlet" else np.ones(nf if name == "c_in" else ne)
        a = np.array(getattr(mesh, name) if getattr(mesh, name) is not None else default, dtype=dtype)
        a[index] = value
        return changed(**{name: a})

    rp = mesh.rowptr.copy()
    rp[1], rp[2] = rp[2], rp[1]
    rp0 = mesh.rowptr.copy()
    rp0[0] = 1
    out = [("n_elem", changed(n_elem=0)), ("n_face", changed(n_face=0)), ("rowptr decreasing", changed(rowptr=rp)),
           ("rowptr[0]", changed(rowptr=rp0)), ("col high", with_entry("col", 3, nf)), ("col negative", with_entry("col", 3, -1)),
           ("val zero", with_entry("val", 2, 0.0)), ("val nan", with_entry("val", 2, np.nan)),
           ("same sign", with_entry("val", pos[0], -mesh.val[pos[0]])),
           ("unequal magnitude", with_entry("val", pos[0], mesh.val[pos[0]] * (1 + 1e-9))),
           ("three entries", with_entry("col", int(np.flatnonzero(mesh.col != interior)[-1]), interior)),
           ("volume zero", with_entry("pore_volume", 1, 0.0)), ("volume negative", with_entry("pore_volume", 1, -1.0)),
           ("volume inf", with_entry("pore_volume", 1, np.inf)), ("c0 nan", with_entry("c0", 0, np.nan, np.float64)),
           ("c_in inf", with_entry("c_in", 0, np.inf, np.float64)), ("weight nan", with_entry("weight", ne - 1, np.nan, np.float64)),
           ("outlet interior", with_entry("outlet", interior, 1, np.uint8))]
    # a dof in no element: drop the last row entry of a boundary dof
    bd = int(np.flatnonzero(s.boundary)[-1])
    q = int(np.flatnonzero(mesh.col == bd)[0])
    rp = mesh.rowptr.copy()
    rp[np.searchsorted(mesh.rowptr, q, side="right"):] -= 1
    out.append(("empty column", changed(rowptr=rp, col=np.delete(mesh.col, q), val=np.delete(mesh.val, q))))
    return out


BAD_PARAMS = [dict(t_end=0.0), dict(t_end=-1.0), dict(cfl=0.0), dict(cfl=1.0 + 1e-12), dict(nreport=0), dict(nreport=4097),
              dict(max_steps=-1), dict(max_steps=2 ** 24 + 1)]
