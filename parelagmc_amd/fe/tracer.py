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


# ---- tangent and adjoint of the walk (the kernels of pmc_tracer_run_adjoint follow them) ----------
# The walk is differentiated with its decisions held: the element sequence, the step count, the chosen exit of every step
# and, for a box, the side of the exit axis.  Clamps are the identity, a coordinate set exactly (the exit plane, the entry
# face's barycentric coordinate) has a zero derivative.
#
# L'(rho) = (1 / (1 + rho) - L) / rho and E'(z) = (e^z - E) / z cancel near zero: below |argument| < 2^-3 they are summed
# as series (Horner), 19 terms of L' = sum_k (-1)^k k rho^(k - 1) / (k + 1) and 11 of E' = sum_k k z^(k - 1) / (k + 1)!.
# At the switch the closed forms lose three bits and the truncated tails are below 2^-56
# (tests/tracer_adjoint_cases.py::derivative_branch_agreement measures both against long double).
_DSERIES = 2.0 ** -3
_LP_TERMS = 19
_EP_TERMS = 11


def _fact(n):
    out = 1
    for i in range(2, n + 1):
        out *= i
    return out


def _Lp(rho):
    """L'(rho) of one scalar, in rho's precision"""
    t = type(rho)
    if abs(rho) < _DSERIES:
        acc = t((-1) ** _LP_TERMS * _LP_TERMS) / t(_LP_TERMS + 1)
        for k in range(_LP_TERMS - 1, 0, -1):
            acc = t((-1) ** k * k) / t(k + 1) + rho * acc
        return acc
    return (1 / (1 + rho) - np.log1p(rho) / rho) / rho


def _Ep(z):
    """E'(z) of one scalar, in z's precision"""
    t = type(z)
    if abs(z) < _DSERIES:
        acc = t(_EP_TERMS) / t(_fact(_EP_TERMS + 1))
        for k in range(_EP_TERMS - 1, 0, -1):
            acc = t(k) / t(_fact(k + 1)) + z * acc
        return acc
    em = np.expm1(z)
    return ((em + 1) - em / z) / z


def _Ls(rho):
    return (1 - rho / 2) + rho * rho / 3 if abs(rho) < _SERIES else np.log1p(rho) / rho


def _Es(z):
    return (1 + z / 2) + z * z / 6 if abs(z) < _SERIES else np.expm1(z) / z


class _Tables:
    """the per-element data of a mesh in one precision"""

    def __init__(self, mesh, dtype):
        self.box = mesh.kind == BOX
        self.nfe = 6 if self.box else 4
        self.face = mesh.elem_face.astype(np.int64)
        self.sgn = mesh.elem_sign.astype(dtype)
        fe = mesh.face_elem.astype(np.int64)
        self.nbr = np.where(fe[self.face, 0] == np.arange(mesh.n_elem)[:, None], fe[self.face, 1], fe[self.face, 0])
        self.phi = np.ones(mesh.n_elem, dtype) if mesh.porosity is None else mesh.porosity.astype(dtype)
        self.geom = mesh.geom.astype(dtype)
        if not self.box:
            self.rows, self.vol = simplex_rows(mesh.geom, dtype)


def _box_velocities(tb, e, F, x):
    lo, hi = tb.geom[e, :3], tb.geom[e, 3:]
    h = hi - lo
    vol = (h[0] * h[1]) * h[2]
    area, vlo, vhi, g, v = [], [], [], [], []
    for a in range(3):
        area.append(vol / h[a])
        vlo.append(-F[_BOX_LO[a]] / area[a])
        vhi.append(F[_BOX_HI[a]] / area[a])
        g.append((vhi[a] - vlo[a]) / h[a])
        v.append(vlo[a] + g[a] * (x[a] - lo[a]))
    return lo, hi, h, area, vlo, vhi, g, v


def _tet_lambda(tb, e, x, dtype):
    r = tb.rows[e]
    return [min(max(((r[i, 0] * x[0] + r[i, 1] * x[1]) + r[i, 2] * x[2]) + r[i, 3], dtype(0)), dtype(1)) for i in range(4)]


def _walk_one(tb, ucol, x0, e0, max_steps, dtype, forced=None):
    """One particle in scalar arithmetic, the operations of `trace` in its order.  Returns (tape, T, x, status, exit_face):
    tape[s] = (element, entry coordinates, exit, side): exit is the axis (box) or the local face (simplex); side is the `up`
    of the exit axis (box) or the local entry face, -1 on the first step (simplex).  forced = (tape, status) of another run
    imposes its decisions (the long-double twin on the float64 path)."""
    inf = dtype(np.inf)
    e = int(e0)
    x = [dtype(c) for c in x0]
    T = dtype(0)
    tape = []
    status, exit_face = MAX_STEPS, -1
    entry = -1
    if tb.box:
        x = [min(max(x[a], tb.geom[e, a]), tb.geom[e, 3 + a]) for a in range(3)]
    else:
        lam = _tet_lambda(tb, e, x, dtype)
    nmax = max_steps if forced is None else len(forced[0])
    for s in range(nmax):
        F = tb.sgn[e] * ucol[tb.face[e]]
        best, which, side = inf, -1, 0
        if tb.box:
            lo, hi, h, area, vlo, vhi, g, v = _box_velocities(tb, e, F, x)
            if forced is None:
                for a in range(3):
                    up = bool(v[a] > 0 and vhi[a] > 0)
                    if up or (v[a] < 0 and vlo[a] < 0):
                        d = hi[a] - x[a] if up else lo[a] - x[a]
                        vex = vhi[a] if up else vlo[a]
                        dt = (d / v[a]) * _Ls((vex - v[a]) / v[a])
                        if dt < best:
                            best, which, side = dt, a, int(up)
            else:
                which, side = forced[0][s][2], forced[0][s][3]
                d = hi[which] - x[which] if side else lo[which] - x[which]
                vex = vhi[which] if side else vlo[which]
                best = (d / v[which]) * _Ls((vex - v[which]) / v[which])
            coords = tuple(x)
        else:
            c3 = 3 * tb.vol[e]
            b = (((F[0] + F[1]) + F[2]) + F[3]) / c3
            w = [F[i] / c3 for i in range(4)]
            vl = [b * lam[i] - w[i] for i in range(4)]
            if forced is None:
                for i in range(4):
                    if F[i] > 0 and vl[i] < 0:
                        dt = (-lam[i] / vl[i]) * _Ls((-w[i] - vl[i]) / vl[i])
                        if dt < best:
                            best, which = dt, i
            else:
                which = forced[0][s][2]
                best = (-lam[which] / vl[which]) * _Ls((-w[which] - vl[which]) / vl[which])
            side = entry
            coords = tuple(lam)
        if which < 0:
            status = STAGNANT
            break
        tape.append((e, coords, which, side))
        T = T + tb.phi[e] * best
        if tb.box:
            for a in range(3):
                c = x[a] + (v[a] * best) * _Es(g[a] * best)
                c = min(max(c, lo[a]), hi[a])
                if a == which:
                    c = hi[a] if side else lo[a]
                x[a] = c
            lf = (_BOX_HI if side else _BOX_LO)[which]
        else:
            eb = _Es(b * best)
            ln = [min(max(lam[i] + (vl[i] * best) * eb, dtype(0)), dtype(1)) for i in range(4)]
            ln[which] = dtype(0)
            V = tb.geom[e]
            x = [V[3, d] + ((ln[0] * (V[0, d] - V[3, d]) + ln[1] * (V[1, d] - V[3, d])) + ln[2] * (V[2, d] - V[3, d]))
                 for d in range(3)]
            lf = which
        f, en = int(tb.face[e, lf]), int(tb.nbr[e, lf])
        if en < 0:
            status, exit_face = EXITED, f
            break
        e = en
        if not tb.box:
            lam = _tet_lambda(tb, e, x, dtype)
            entry = int(np.nonzero(tb.face[e] == f)[0][0])
            lam[entry] = dtype(0)
    if forced is not None:
        status = forced[1]
    return tape, T, x, status, exit_face


def _step_values(tb, step, F):
    """the forward values of one recorded step that its derivatives need"""
    e, c, which, side = step
    if tb.box:
        lo, hi, h, area, vlo, vhi, g, v = _box_velocities(tb, e, F, c)
        d = hi[which] - c[which] if side else lo[which] - c[which]
        vex = vhi[which] if side else vlo[which]
        q = d / v[which]
        rho = (vex - v[which]) / v[which]
        Lr = _Ls(rho)
        return dict(lo=lo, h=h, area=area, g=g, v=v, q=q, rho=rho, Lr=Lr, dt=q * Lr)
    c3 = 3 * tb.vol[e]
    b = (((F[0] + F[1]) + F[2]) + F[3]) / c3
    w = [F[i] / c3 for i in range(4)]
    v = [b * c[i] - w[i] for i in range(4)]
    q = -c[which] / v[which]
    rho = (-w[which] - v[which]) / v[which]
    Lr = _Ls(rho)
    dt = q * Lr
    return dict(c3=c3, b=b, v=v, q=q, rho=rho, Lr=Lr, dt=dt, z=b * dt, eb=_Es(b * dt))


def _step_adjoint(tb, step, F, Tbar, xbar, dtype):
    """One step backwards: from the adjoints of T and of the position after the step to (Fbar (nfe), the adjoint of the
    entry coordinates).  csrc/tracer.hip performs these operations in this order."""
    e, c, A, side = step
    m = _step_values(tb, step, F)
    zero = dtype(0)
    dt, q, rho, Lr, v = m["dt"], m["q"], m["rho"], m["Lr"], m["v"]
    dtb = tb.phi[e] * Tbar
    if tb.box:
        g, lo, h, area = m["g"], m["lo"], m["h"], m["area"]
        vb, gb, xin = [zero] * 3, [zero] * 3, [zero] * 3
        for a in range(3):
            if a == A:
                continue
            z = g[a] * dt
            cb = xbar[a]
            mb = cb * _Es(z)
            zb = (cb * (v[a] * dt)) * _Ep(z)
            xin[a] = cb
            vb[a] = mb * dt
            gb[a] = zb * dt
            dtb = dtb + mb * v[a]
            dtb = dtb + zb * g[a]
        qb = dtb * Lr
        rb = (dtb * q) * _Lp(rho)
        vexb = rb / v[A]
        vb[A] = -(qb * q) / v[A] - (rb * (1 + rho)) / v[A]
        xin[A] = -(qb / v[A])
        Fb = [zero] * 6
        for a in range(3):
            gba = gb[a] + vb[a] * (c[a] - lo[a])
            xin[a] = xin[a] + vb[a] * g[a]
            vlob = vb[a] - gba / h[a]
            vhib = gba / h[a]
            if a == A:
                if side:
                    vhib = vhib + vexb
                else:
                    vlob = vlob + vexb
            Fb[_BOX_LO[a]] = -vlob / area[a]
            Fb[_BOX_HI[a]] = vhib / area[a]
        return Fb, xin
    V = tb.geom[e]
    b, eb, z, c3 = m["b"], m["eb"], m["z"], m["c3"]
    lnb = [(((V[j, 0] - V[3, 0]) * xbar[0] + (V[j, 1] - V[3, 1]) * xbar[1]) + (V[j, 2] - V[3, 2]) * xbar[2]) for j in range(3)]
    lnb.append(zero)
    lnb[A] = zero
    lamb, vb, wb = [zero] * 4, [zero] * 4, [zero] * 4
    ebb = zero
    for i in range(4):
        mb = lnb[i] * eb
        ebb = ebb + lnb[i] * (v[i] * dt)
        lamb[i] = lnb[i]
        vb[i] = mb * dt
        dtb = dtb + mb * v[i]
    zb = ebb * _Ep(z)
    bb = zb * dt
    dtb = dtb + zb * b
    qb = dtb * Lr
    rb = (dtb * q) * _Lp(rho)
    lamb[A] = lamb[A] - qb / v[A]
    vb[A] = (vb[A] - (qb * q) / v[A]) - (rb * (1 + rho)) / v[A]
    wb[A] = -(rb / v[A])
    for i in range(4):
        bb = bb + vb[i] * c[i]
        lamb[i] = lamb[i] + vb[i] * b
        wb[i] = wb[i] - vb[i]
    return [(wb[i] + bb) / c3 for i in range(4)], lamb


def _rows_transpose(tb, e, lamb, skip):
    """adjoint of lambda_k = row_k . x + d_k over the faces k != skip"""
    r = tb.rows[e]
    lb = [lamb[k] if k != skip else type(lamb[k])(0) for k in range(4)]
    return [((r[0, d] * lb[0] + r[1, d] * lb[1]) + r[2, d] * lb[2]) + r[3, d] * lb[3] for d in range(3)]


def _step_tangent(tb, step, F, dF, dc, dtype):
    """One step forwards: from the tangents of the outward fluxes and of the entry coordinates to (d dt, the tangent of the
    position (box) / of the position through the barycentric coordinates (simplex))"""
    e, c, A, side = step
    m = _step_values(tb, step, F)
    dt, q, rho, Lr, v = m["dt"], m["q"], m["rho"], m["Lr"], m["v"]
    zero = dtype(0)
    if tb.box:
        g, lo, h, area = m["g"], m["lo"], m["h"], m["area"]
        dv, dg, dvlo, dvhi = [], [], [], []
        for a in range(3):
            dvlo.append(-dF[_BOX_LO[a]] / area[a])
            dvhi.append(dF[_BOX_HI[a]] / area[a])
            dg.append((dvhi[a] - dvlo[a]) / h[a])
            dv.append(dvlo[a] + dg[a] * (c[a] - lo[a]) + g[a] * dc[a])
        dvex = dvhi[A] if side else dvlo[A]
        dq = (-dc[A] - q * dv[A]) / v[A]
        drho = (dvex - (1 + rho) * dv[A]) / v[A]
        ddt = dq * Lr + q * _Lp(rho) * drho
        out = []
        for a in range(3):
            z = g[a] * dt
            out.append(zero if a == A else dc[a] + (dv[a] * dt + v[a] * ddt) * _Es(z)
                       + (v[a] * dt) * _Ep(z) * (dg[a] * dt + g[a] * ddt))
        return ddt, out
    b, eb, z, c3 = m["b"], m["eb"], m["z"], m["c3"]
    db = (((dF[0] + dF[1]) + dF[2]) + dF[3]) / c3
    dv = [db * c[i] + b * dc[i] - dF[i] / c3 for i in range(4)]
    dq = (-dc[A] - q * dv[A]) / v[A]
    drho = (-dF[A] / c3 - (1 + rho) * dv[A]) / v[A]
    ddt = dq * Lr + q * _Lp(rho) * drho
    deb = _Ep(z) * (db * dt + b * ddt)
    dln = [zero if i == A else dc[i] + (dv[i] * dt + v[i] * ddt) * eb + (v[i] * dt) * deb for i in range(4)]
    V = tb.geom[e]
    return ddt, [(dln[0] * (V[0, d] - V[3, d]) + dln[1] * (V[1, d] - V[3, d])) + dln[2] * (V[2, d] - V[3, d]) for d in range(3)]


def _prepare(mesh, u, x0, elem0, max_steps, dtype, decisions):
    u2 = np.atleast_2d(np.asarray(u, dtype=dtype))
    if max_steps == 0:
        max_steps = default_max_steps(mesh.n_elem)
    tb = _Tables(mesh, dtype)
    x0 = np.asarray(x0, dtype=dtype).reshape(-1, 3)
    paths = []
    for b in range(u2.shape[0]):
        for p in range(len(elem0)):
            forced = None if decisions is None else decisions[b][p]
            paths.append(_walk_one(tb, u2[b], x0[p], elem0[p], max_steps, dtype, forced))
    return u2, tb, paths


def _forward_dict(paths, nb, npart, dtype, squeeze):
    res = dict(T=np.array([p[1] for p in paths], dtype).reshape(nb, npart),
               exit_face=np.array([p[4] for p in paths], np.int32).reshape(nb, npart),
               status=np.array([p[3] for p in paths], np.int32).reshape(nb, npart),
               nsteps=np.array([len(p[0]) for p in paths], np.int32).reshape(nb, npart),
               x_exit=np.array([p[2] for p in paths], dtype).reshape(nb, npart, 3))
    res["decisions"] = [[(paths[b * npart + p][0], paths[b * npart + p][3]) for p in range(npart)] for b in range(nb)]
    if squeeze:
        res = {k: v[0] for k, v in res.items()}
    return res


def trace_tangent(mesh: TracerMesh, u, du, x0, elem0, max_steps=0, dtype=np.float64, dx0=None, decisions=None):
    """Directional derivative of `trace` for the flux direction du (the shape of u) and, optionally, the start-point
    direction dx0 (nparticles, 3), the decisions of the walk held.  Returns trace's forward outputs (without the margin) and
    dT, dx_exit; particles that did not exit get zeros.  decisions: the "decisions" entry of another call's result (always
    with the batch axis) imposes that call's path - the long-double reference on the float64 path."""
    u2, tb, paths = _prepare(mesh, u, x0, elem0, max_steps, dtype, decisions)
    du2 = np.atleast_2d(np.asarray(du, dtype=dtype))
    nb, npart = u2.shape[0], len(elem0)
    dx0 = np.zeros((npart, 3), dtype) if dx0 is None else np.asarray(dx0, dtype=dtype).reshape(npart, 3)
    dT = np.zeros((nb, npart), dtype)
    dxe = np.zeros((nb, npart, 3), dtype)
    for b in range(nb):
        for p in range(npart):
            tape, _, _, status, _ = paths[b * npart + p]
            if status != EXITED:
                continue
            acc = dtype(0)
            dx = [dx0[p, d] for d in range(3)]
            for s, step in enumerate(tape):
                e = step[0]
                F = tb.sgn[e] * u2[b, tb.face[e]]
                dF = tb.sgn[e] * du2[b, tb.face[e]]
                if tb.box:
                    dc = dx
                else:
                    r = tb.rows[e]
                    dc = [dtype(0) if k == step[3] else (r[k, 0] * dx[0] + r[k, 1] * dx[1]) + r[k, 2] * dx[2] for k in range(4)]
                ddt, dx = _step_tangent(tb, step, F, dF, dc, dtype)
                acc = acc + tb.phi[e] * ddt
            dT[b, p] = acc
            dxe[b, p] = dx
    res = _forward_dict(paths, nb, npart, dtype, False)
    res.update(dT=dT, dx_exit=dxe)
    if np.ndim(u) == 1:
        res = {k: v[0] for k, v in res.items()}
    return res


def trace_adjoint(mesh: TracerMesh, u, x0, elem0, T_bar=None, x_exit_bar=None, max_steps=0, dtype=np.float64, decisions=None):
    """Numpy twin of pmc_tracer_run_adjoint: u_bar (nbatch, n_face) and x0_bar (nbatch, nparticles, 3) of
    J = <T_bar, T> + <x_exit_bar, x_exit> per column, the decisions of the walk held, with trace's forward outputs (T,
    exit_face, status, nsteps, x_exit: the same bits).  Particles that did not exit contribute nothing.

    u_bar[f] is summed from 0.0 over the elements of face_elem[f] in that order and, within an element, over the visits in
    ascending (particle, step)."""
    u2, tb, paths = _prepare(mesh, u, x0, elem0, max_steps, dtype, decisions)
    nb, npart = u2.shape[0], len(elem0)
    Tb = np.zeros((nb, npart), dtype) if T_bar is None else np.asarray(T_bar, dtype=dtype).reshape(nb, npart)
    xb = np.zeros((nb, npart, 3), dtype) if x_exit_bar is None else np.asarray(x_exit_bar, dtype=dtype).reshape(nb, npart, 3)
    ubar = np.zeros((nb, mesh.n_face), dtype)
    x0bar = np.zeros((nb, npart, 3), dtype)
    local = {}
    for e in range(mesh.n_elem):
        for l in range(tb.nfe):
            local[e, int(tb.face[e, l])] = l
    for b in range(nb):
        visits = {}                                        # element -> [(particle, step, Fbar)]
        for p in range(npart):
            tape, _, _, status, _ = paths[b * npart + p]
            if status != EXITED:
                continue
            xbar = [xb[b, p, d] for d in range(3)]
            for s in range(len(tape) - 1, -1, -1):
                step = tape[s]
                e = step[0]
                F = tb.sgn[e] * u2[b, tb.face[e]]
                Fb, cin = _step_adjoint(tb, step, F, Tb[b, p], xbar, dtype)
                visits.setdefault(e, []).append((p, s, Fb))
                xbar = cin if tb.box else _rows_transpose(tb, e, cin, step[3])
            x0bar[b, p] = xbar
        for e in visits:
            visits[e].sort(key=lambda t: (t[0], t[1]))
        for f in range(mesh.n_face):
            acc = dtype(0)
            for e in mesh.face_elem[f]:
                if e < 0 or int(e) not in visits:
                    continue
                l = local[int(e), f]
                for _, _, Fb in visits[int(e)]:
                    acc = acc + tb.sgn[e, l] * Fb[l]
            ubar[b, f] = acc
    res = _forward_dict(paths, nb, npart, dtype, False)
    res.update(u_bar=ubar, x0_bar=x0bar)
    if np.ndim(u) == 1:
        res = {k: v[0] for k, v in res.items()}
    return res


def reduce_seed(T, status, kind=MEAN):
    """Twin of pmc_tracer_reduce_seed: T_bar = dQ/dT of the Q of `reduce`.  MEAN: 1 / nparticles on the particles that exited;
    MIN: 1 on the lowest-index particle attaining the minimum, if it exited; 0 elsewhere."""
    T, status = np.atleast_2d(T), np.atleast_2d(status)
    out = np.zeros(T.shape)
    if kind == MEAN:
        out[status == EXITED] = 1.0 / T.shape[1]
    else:
        j = T.argmin(axis=1)
        r = np.arange(T.shape[0])
        out[r, j] = (status[r, j] == EXITED).astype(np.float64)
    return out
