"""Particle travel times on the RT0 Darcy flux: setup arrays and the numpy twin of csrc/tracer.hip.

Inside an element the RT0 velocity is affine, so every coordinate c (a box axis, a barycentric coordinate of a simplex)
obeys c' = v(c) with v affine in c and the time to a candidate exit plane is closed-form (Pollock's method):

    dt = (d / v) L(rho),   rho = (v_exit - v) / v,   L(rho) = log1p(rho) / rho.

`trace` below is the reference the kernel follows operation for operation; it additionally returns the decision margin of
every particle (the smallest relative gap between the two earliest exit candidates along its path).
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np

from .mesh import _LOCAL_FACES
from .rt0 import LevelSpaces

BOX, SIMPLEX = 0, 1                      # pmc_tracer_mesh.kind
EXITED, STAGNANT, MAX_STEPS = 0, 1, 2    # status of a path
MEAN, MIN = 0, 1                         # QoI kinds of pmc_tracer_reduce / pmc_darcy_set_tracer

# local faces of a hexahedron on the low / high side of the axes x, y, z (fe/mesh.py: z-, y-, x+, y+, x-, z+)
_BOX_LO = (4, 1, 0)
_BOX_HI = (2, 3, 5)
_SERIES = 2.0 ** -20                     # |argument| below which L and E switch to their series


@dataclasses.dataclass
class TracerMesh:
    kind: int
    n_elem: int
    n_face: int
    elem_face: np.ndarray          # (n_elem, n_fe) int32
    elem_sign: np.ndarray          # (n_elem, n_fe) int8
    face_elem: np.ndarray          # (n_face, 2) int32
    geom: np.ndarray               # BOX (n_elem, 6) lo, hi; SIMPLEX (n_elem, 4, 3) vertices
    porosity: Optional[np.ndarray] = None


def tracer_mesh(level_spaces: LevelSpaces, porosity=None) -> TracerMesh:
    """The arrays of pmc_tracer_mesh from one level's mesh and face table (3-D meshes with element geometry only)."""
    m, ft = level_spaces.mesh, level_spaces.faces
    if m.etype == "hex":
        p = m.verts[m.elems]
        lo, hi = p.min(axis=1), p.max(axis=1)
        if (np.abs(np.prod(hi - lo, axis=1) - level_spaces.vol) > 1e-10 * level_spaces.vol).any():
            raise ValueError("tracer_mesh: hexahedra must be axis-aligned boxes")
        # every vertex of a box is a corner of its bounding box
        if not np.all((p == lo[:, None, :]) | (p == hi[:, None, :])):
            raise ValueError("tracer_mesh: hexahedra must be axis-aligned boxes")
        kind, geom = BOX, np.concatenate([lo, hi], axis=1)
    elif m.etype == "tet":
        kind, geom = SIMPLEX, m.verts[m.elems].copy()
    else:
        raise ValueError("tracer_mesh: only 3-D meshes of hexahedra or tetrahedra carry a tracer")
    phi = None
    if porosity is not None:
        phi = np.ascontiguousarray(np.broadcast_to(np.asarray(porosity, np.float64), (m.ne,)))
        if not (phi > 0).all():
            raise ValueError("tracer_mesh: porosity must be positive")
    return TracerMesh(kind, m.ne, ft.face_verts.shape[0], np.ascontiguousarray(ft.elem_face, np.int32),
                      np.ascontiguousarray(ft.elem_sign, np.int8), np.ascontiguousarray(ft.face_elem, np.int32),
                      np.ascontiguousarray(geom, np.float64), phi)


def default_max_steps(n_elem: int) -> int:
    """64 + 32 ceil(cbrt(n_elem)), in integers"""
    c = 0
    while c * c * c < n_elem:
        c += 1
    return 64 + 32 * c


def simplex_rows(verts, dtype=np.float64):
    """(rows (ne, 4, 4), vol (ne,)): lambda_i(x) = rows[e, i, :3] . x + rows[e, i, 3] and |e|, by cross products in the order
    csrc/tracer.hip uses (local face i, opposite vertex i, has the vertices _LOCAL_FACES['tet'][i] with outward normal)."""
    V = np.asarray(verts, dtype=dtype)
    e1, e2, e3 = V[:, 1] - V[:, 0], V[:, 2] - V[:, 0], V[:, 3] - V[:, 0]
    vol6 = _dot3(_cross(e1, e2), e3)
    rows = np.empty((V.shape[0], 4, 4), dtype=dtype)
    for i in range(4):
        a, b, c = _LOCAL_FACES["tet"][i]
        n = _cross(V[:, b] - V[:, a], V[:, c] - V[:, a])
        g = -n / vol6[:, None]
        rows[:, i, :3] = g
        rows[:, i, 3] = -_dot3(g, V[:, a])
    return rows, vol6 / 6


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def locate(mesh: TracerMesh, points) -> np.ndarray:
    """Start elements of `points` (npoints x 3), found geometrically: among the elements whose bounding box holds the point,
    the one whose smallest barycentric coordinate / relative distance to its box faces is largest.  Raises when a point lies
    outside every element.  (No index arithmetic: the elements of a refined level are not numbered x-fastest.)"""
    pts = np.atleast_2d(np.asarray(points, np.float64))
    out = np.empty(len(pts), np.int32)
    if mesh.kind == BOX:
        lo, hi = mesh.geom[:, :3], mesh.geom[:, 3:]
    else:
        rows, _ = _rows_cached(mesh)
        lo, hi = mesh.geom.min(axis=1), mesh.geom.max(axis=1)
    pad = 1e-12 * (hi - lo)
    for j, x in enumerate(pts):
        cand = np.nonzero(np.all((lo - pad <= x) & (x <= hi + pad), axis=1))[0]
        if len(cand) == 0:
            raise ValueError("locate: a point lies outside the mesh")
        if mesh.kind == BOX:
            score = (np.minimum(x - lo[cand], hi[cand] - x) / (hi[cand] - lo[cand])).min(axis=1)
        else:
            score = (rows[cand, :, :3] @ x + rows[cand, :, 3]).min(axis=1)
        if score.max() < -1e-12:
            raise ValueError("locate: a point lies outside the mesh")
        out[j] = cand[score.argmax()]
    return out


def velocity(mesh: TracerMesh, u, x):
    """RT0 velocity u_h(x) / porosity at one point (the right-hand side an ODE integrator sees): the element is the one
    `locate` scores best, also for a point slightly outside the mesh."""
    x = np.asarray(x, np.float64)
    if mesh.kind == BOX:
        lo, hi = mesh.geom[:, :3], mesh.geom[:, 3:]
        e = int((np.minimum(x - lo, hi - x) / (hi - lo)).min(axis=1).argmax())
        h = hi[e] - lo[e]
        F = mesh.elem_sign[e] * np.asarray(u)[mesh.elem_face[e]]
        v = np.empty(3)
        for a in range(3):
            area = h.prod() / h[a]
            vlo, vhi = -F[_BOX_LO[a]] / area, F[_BOX_HI[a]] / area
            v[a] = vlo + (vhi - vlo) / h[a] * (x[a] - lo[e, a])
    else:
        rows, vol = _rows_cached(mesh)
        e = int((rows[:, :, :3] @ x + rows[:, :, 3]).min(axis=1).argmax())
        F = mesh.elem_sign[e] * np.asarray(u)[mesh.elem_face[e]]
        v = (F[:, None] * (x[None, :] - mesh.geom[e])).sum(axis=0) / (3 * vol[e])
    return v / (1.0 if mesh.porosity is None else mesh.porosity[e])


def _rows_cached(mesh):
    if getattr(mesh, "_rows", None) is None:
        mesh._rows = simplex_rows(mesh.geom)
    return mesh._rows


def _L(rho):
    small = np.abs(rho) < _SERIES
    safe = np.where(small, 1, rho)
    return np.where(small, (1 - rho / 2) + rho * rho / 3, np.log1p(safe) / safe)


def _E(z):
    small = np.abs(z) < _SERIES
    safe = np.where(small, 1, z)
    return np.where(small, (1 + z / 2) + z * z / 6, np.expm1(safe) / safe)


def _pick(best, second, which, dt, tag):
    """running smallest / second smallest candidate time, in candidate order (ties keep the earlier candidate)"""
    first = dt < best
    nsecond = np.where(first, best, np.where(dt < second, dt, second))
    return np.where(first, dt, best), nsecond, np.where(first, tag, which)


def trace(mesh: TracerMesh, u, x0, elem0, max_steps=0, dtype=np.float64):
    """Numpy twin of pmc_tracer_run.  u: (n_face,) or (nbatch, n_face) fluxes in the direction of the faces' global normals;
    x0 (nparticles, 3), elem0 (nparticles,).  Returns a dict of (nbatch, nparticles) arrays T, exit_face, status, nsteps,
    margin and x_exit (nbatch, nparticles, 3); a one-dimensional u drops the batch axis.  dtype: the arithmetic
    (np.float64, or np.longdouble for the rounding-error reference)."""
    u2 = np.atleast_2d(np.asarray(u, dtype=dtype))
    nb, npart = u2.shape[0], len(elem0)
    if max_steps == 0:
        max_steps = default_max_steps(mesh.n_elem)
    inf = dtype(np.inf)
    box = mesh.kind == BOX
    nfe = 6 if box else 4
    face = mesh.elem_face.astype(np.int64)
    sgn = mesh.elem_sign.astype(dtype)
    fe = mesh.face_elem.astype(np.int64)
    nbr = np.where(fe[face, 0] == np.arange(mesh.n_elem)[:, None], fe[face, 1], fe[face, 0])   # (n_elem, nfe)
    phi = np.ones(mesh.n_elem, dtype) if mesh.porosity is None else mesh.porosity.astype(dtype)
    geom = mesh.geom.astype(dtype)
    if not box:
        rows, vol = simplex_rows(mesh.geom, dtype)
    N = nb * npart
    bidx = np.repeat(np.arange(nb), npart)
    e = np.tile(np.asarray(elem0, np.int64), nb)
    x = np.tile(np.asarray(x0, dtype=dtype), (nb, 1))
    T = np.zeros(N, dtype)
    status = np.full(N, MAX_STEPS, np.int32)
    exit_face = np.full(N, -1, np.int32)
    nsteps = np.zeros(N, np.int32)
    margin = np.full(N, np.inf)
    active = np.ones(N, bool)
    if box:
        x = np.minimum(np.maximum(x, geom[e, :3]), geom[e, 3:])
    else:
        lam = np.minimum(np.maximum(_lambda(rows, e, x), 0), 1)
    with np.errstate(all="ignore"):
        for _ in range(max_steps):
            idx = np.nonzero(active)[0]
            if len(idx) == 0:
                break
            ei, bi = e[idx], bidx[idx]
            F = sgn[ei] * u2[bi[:, None], face[ei]]                       # outward fluxes (n, nfe)
            best = np.full(len(idx), inf, dtype)
            second = np.full(len(idx), inf, dtype)
            which = np.full(len(idx), -1, np.int64)                       # local exit face
            if box:
                xi = x[idx]
                lo, hi = geom[ei, :3], geom[ei, 3:]
                h = hi - lo
                vol_e = (h[:, 0] * h[:, 1]) * h[:, 2]
                vs, gs = [], []
                for a in range(3):
                    area = vol_e / h[:, a]
                    vlo, vhi = -F[:, _BOX_LO[a]] / area, F[:, _BOX_HI[a]] / area
                    g = (vhi - vlo) / h[:, a]
                    v = vlo + g * (xi[:, a] - lo[:, a])
                    up = (v > 0) & (vhi > 0)
                    cand = up | ((v < 0) & (vlo < 0))
                    d = np.where(up, hi[:, a] - xi[:, a], lo[:, a] - xi[:, a])
                    vex = np.where(up, vhi, vlo)
                    vsafe = np.where(cand, v, 1)
                    dt = np.where(cand, (d / vsafe) * _L((vex - vsafe) / vsafe), inf)
                    best, second, which = _pick(best, second, which, dt, np.where(up, _BOX_HI[a], _BOX_LO[a]))
                    vs.append(v)
                    gs.append(g)
            else:
                li = lam[idx]
                c3 = 3 * vol[ei]
                b = (((F[:, 0] + F[:, 1]) + F[:, 2]) + F[:, 3]) / c3
                w = F / c3[:, None]
                vl = b[:, None] * li - w
                for i in range(4):
                    cand = (F[:, i] > 0) & (vl[:, i] < 0)
                    vsafe = np.where(cand, vl[:, i], 1)
                    dt = np.where(cand, (-li[:, i] / vsafe) * _L((-w[:, i] - vsafe) / vsafe), inf)
                    best, second, which = _pick(best, second, which, dt, i)
            go = which >= 0
            stag = idx[~go]
            status[stag] = STAGNANT
            active[stag] = False
            idx, ei, bi, best, second, which = idx[go], ei[go], bi[go], best[go], second[go], which[go]
            if len(idx) == 0:
                continue
            mg = np.where(np.isinf(second), np.inf, (second - best) / best)
            mg = np.where(np.isnan(mg), 0.0, mg).astype(np.float64)
            margin[idx] = np.minimum(margin[idx], mg)
            T[idx] += phi[ei] * best
            nsteps[idx] += 1
            r = np.arange(len(idx))
            if box:
                xn = np.empty((len(idx), 3), dtype)
                for a in range(3):
                    v, g = vs[a][go], gs[a][go]
                    c = xi[go, a] + (v * best) * _E(g * best)
                    c = np.minimum(np.maximum(c, lo[go, a]), hi[go, a])
                    c = np.where(which == _BOX_HI[a], hi[go, a], c)
                    xn[:, a] = np.where(which == _BOX_LO[a], lo[go, a], c)
                x[idx] = xn
            else:
                ln = li[go] + (vl[go] * best[:, None]) * _E(b[go] * best)[:, None]
                ln = np.minimum(np.maximum(ln, 0), 1)
                ln[r, which] = 0
                # the position relative to vertex 3: a coordinate set to zero or clamped (sum lambda != 1 by eta) then moves
                # it by eta x an edge, not by eta x a vertex's distance from the origin - the latter grows by |V| / h per
                # element and throws the particle out of the mesh within a dozen steps
                V = geom[ei]
                x[idx] = V[:, 3] + ((ln[:, 0, None] * (V[:, 0] - V[:, 3]) + ln[:, 1, None] * (V[:, 1] - V[:, 3]))
                                    + ln[:, 2, None] * (V[:, 2] - V[:, 3]))
                lam[idx] = ln
            f = face[ei, which]
            en = nbr[ei, which]
            out = en < 0
            status[idx[out]] = EXITED
            exit_face[idx[out]] = f[out]
            active[idx[out]] = False
            mv = ~out
            e[idx[mv]] = en[mv]
            if not box and mv.any():
                im, em = idx[mv], en[mv]
                ln = np.minimum(np.maximum(_lambda(rows, em, x[im]), 0), 1)
                ln[face[em] == f[mv][:, None]] = 0                        # the entry face: lambda = 0 exactly
                lam[im] = ln
    res = dict(T=T.reshape(nb, npart), exit_face=exit_face.reshape(nb, npart), status=status.reshape(nb, npart),
               nsteps=nsteps.reshape(nb, npart), margin=margin.reshape(nb, npart), x_exit=x.reshape(nb, npart, 3),
               elem=e.reshape(nb, npart).astype(np.int32))
    if np.ndim(u) == 1:
        res = {k: v[0] for k, v in res.items()}
    return res


def _lambda(rows, e, x):
    r = rows[e]                                                           # (n, 4, 4)
    return ((r[:, :, 0] * x[:, None, 0] + r[:, :, 1] * x[:, None, 1]) + r[:, :, 2] * x[:, None, 2]) + r[:, :, 3]


def reduce(T, status, kind=MEAN):
    """Twin of pmc_tracer_reduce up to the summation order: (Q (nbatch,), not_exited (nbatch,))"""
    T = np.atleast_2d(T)
    q = T.mean(axis=1) if kind == MEAN else T.min(axis=1)
    return q, (np.atleast_2d(status) != EXITED).sum(axis=1).astype(np.int32)
