"""First-order upwind transport of a passive solute on the Darcy flux: mesh arrays from a level's divergence matrix and the
numpy twin of csrc/transport.hip (pmc_transport_*).

The scheme needs no geometry: the rows of B (n_elem x n_face, not eliminated) say which flux dofs bound an element and with
which sign, the flux block of a solve gives the volume rate through each, and one pore volume per element turns rates into
concentrations.  A dof f of B has one entry (boundary) or two of opposite sign and equal magnitude (interior); its magnitude
a_f is that of its lowest element, and the outward rate of element e through its l-th row entry is
    g_l = sign(B[e, f]) * (a_f * u_f),
so both elements of an interior dof see the same product.  Per realization
    out_e = sum_l max(g_l, 0),  in_e = sum_l max(-g_l, 0),  r_e = max(out_e, in_e),  rate = max_e r_e / V_e
    x = (t_end * rate) / cfl,  nsteps = max(1, ceil(x)),  dt = t_end / nsteps,  w_e = dt / V_e,  d_e = 1 - w_e r_e
    c_e' = d_e c_e + w_e sum_l max(-g_l, 0) cn_l         (cn_l: the neighbour's old c, c_in[f] on a boundary dof)
with every sum started at 0.0 and taken in ascending l.  The twin restates the kernel operation for operation (numpy forms no
fused multiply-adds; the kernel file switches them off), also in np.longdouble.

A row with a non-finite g makes r_e / V_e count as +inf, so rate is +inf and the column's status BAD_FLUX (numpy's maximum
would carry a NaN along, the device's fmax would drop it: both are told what to do instead).

ceil is the scheme's only decision.  Its margin is |x - r| / max(x, 1) with r the integer nearest to x, but at least 1: below
x = 1 the step count is 1 whatever x is, so a column of zero flux (x = 0) decides nothing and has margin 1.

advance_adjoint and advance_tangent (the end of this file) are the discrete adjoint and the linearisation of advance in u with
the step count, the sign of every g and the branch of max(out_e, in_e) held fixed: the twin of pmc_transport_run_adjoint
(DESIGN.md section 23)."""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np
import scipy.sparse as sp

OK, STEP_LIMIT, BAD_FLUX = 0, 1, 2
MASS_OUT, STORED = 0, 1
DEFAULT_MAX_STEPS = 65536
_THREADS = 256


@dataclasses.dataclass
class TransportMesh:
    """the arrays of pmc_transport_mesh; None where the C struct takes NULL"""
    n_elem: int
    n_face: int
    rowptr: np.ndarray
    col: np.ndarray
    val: np.ndarray
    pore_volume: np.ndarray
    c0: Optional[np.ndarray] = None
    c_in: Optional[np.ndarray] = None
    outlet: Optional[np.ndarray] = None
    weight: Optional[np.ndarray] = None


@dataclasses.dataclass
class Structure:
    """what create derives from the mesh: padded rows and the outlet list"""
    width: int
    face: np.ndarray        # (n_elem, width) dof of the l-th row entry, 0 where padded
    sign: np.ndarray        # (n_elem, width) +1 / -1, 0 where padded
    nbr: np.ndarray         # (n_elem, width) the other element, -1 on the boundary and where padded
    mask: np.ndarray        # (n_elem, width) a real entry
    a: np.ndarray           # (n_face,) magnitudes
    boundary: np.ndarray    # (n_face,) bool
    out_elem: np.ndarray    # (n_outlet,) element and row slot of every outlet dof, ascending dof
    out_slot: np.ndarray
    out_face: np.ndarray
    c0: np.ndarray
    c_in: np.ndarray
    weight: np.ndarray


def validate(m: TransportMesh) -> Structure:
    """Raises ValueError on exactly what pmc_transport_create refuses; returns the derived structure."""
    ne, nf = int(m.n_elem), int(m.n_face)
    if ne < 1 or nf < 1:
        raise ValueError("transport: empty mesh")
    for name in ("rowptr", "col", "val", "pore_volume"):
        if getattr(m, name) is None:
            raise ValueError(f"transport: {name} is missing")
    rowptr, col, val = np.asarray(m.rowptr, np.int64), np.asarray(m.col, np.int64), np.asarray(m.val, np.float64)
    if rowptr.shape != (ne + 1,) or rowptr[0] != 0 or (np.diff(rowptr) < 0).any() or rowptr[-1] != col.size or col.size != val.size:
        raise ValueError("transport: bad rowptr")
    if col.size and (col.min() < 0 or col.max() >= nf):
        raise ValueError("transport: column index out of range")
    if not np.isfinite(val).all() or (val == 0.0).any():
        raise ValueError("transport: B holds a zero or non-finite entry")
    V = np.asarray(m.pore_volume, np.float64)
    if V.shape != (ne,) or not np.isfinite(V).all() or (V <= 0).any():
        raise ValueError("transport: pore volumes must be positive and finite")
    row = np.repeat(np.arange(ne), np.diff(rowptr))
    count = np.bincount(col, minlength=nf)
    if ((count < 1) | (count > 2)).any():
        raise ValueError("transport: a column of B must have one or two entries")
    # entries by column, ascending element within a column (CSR order is ascending row)
    order = np.argsort(col, kind="stable")
    start = np.concatenate([[0], np.cumsum(count)])
    first = order[start[:-1]]
    last = order[start[1:] - 1]
    interior = count == 2
    va, vb = val[first], val[last]
    bad = interior & ((row[first] == row[last]) | (va * vb > 0) | (np.abs(va + vb) > 1e-12 * np.maximum(np.abs(va), np.abs(vb))))
    if bad.any():
        raise ValueError("transport: the two entries of a column of B must lie in two elements, with opposite signs and equal "
                         "magnitudes")
    a = np.abs(va)
    other = np.full(col.size, -1, np.int64)
    other[first[interior]] = row[last[interior]]
    other[last[interior]] = row[first[interior]]
    def opt(x, n, fill, what):
        if x is None:
            return np.full(n, fill, np.float64)
        x = np.asarray(x, np.float64)
        if x.shape != (n,) or not np.isfinite(x).all():
            raise ValueError(f"transport: {what} must be finite")
        return x
    c0 = opt(m.c0, ne, 0.0, "c0")
    c_in = opt(m.c_in, nf, 1.0, "c_in")
    weight = V.copy() if m.weight is None else opt(m.weight, ne, 0.0, "weight")
    boundary = ~interior
    if m.outlet is None:
        outlet = boundary
    else:
        outlet = np.asarray(m.outlet).astype(bool)
        if outlet.shape != (nf,) or (outlet & interior).any():
            raise ValueError("transport: an outlet flag on an interior dof")
    width = int(np.diff(rowptr).max())
    slot = np.arange(col.size) - rowptr[row]
    face = np.zeros((ne, width), np.int64)
    sign = np.zeros((ne, width))
    nbr = np.full((ne, width), -1, np.int64)
    mask = np.zeros((ne, width), bool)
    face[row, slot], sign[row, slot], nbr[row, slot], mask[row, slot] = col, np.sign(val), other, True
    of = np.flatnonzero(outlet)
    return Structure(width, face, sign, nbr, mask, a, boundary, row[first[of]], slot[first[of]], of, c0, c_in, weight)


def transport_mesh(level, volumes, porosity=1.0, outlet=None, c_in=None, c0=None, weight=None) -> TransportMesh:
    """The transport arrays of a Darcy level (anything with the divergence matrix `B`, n_elem x n_face, not eliminated):
    pore volumes porosity * volumes.  Raises ValueError on exactly what pmc_transport_create refuses - a level whose B has
    columns of more than two entries or of unequal magnitudes (a smoothed prolongator, non-unit weights in P_s) among them."""
    B = sp.csr_matrix(level.B)
    B.sort_indices()
    f64 = lambda x: None if x is None else np.ascontiguousarray(x, np.float64)
    m = TransportMesh(B.shape[0], B.shape[1], B.indptr.astype(np.int32), B.indices.astype(np.int32), B.data.astype(np.float64),
                      np.ascontiguousarray(np.asarray(porosity, np.float64) * np.asarray(volumes, np.float64)), f64(c0), f64(c_in),
                      None if outlet is None else np.ascontiguousarray(outlet, np.uint8), f64(weight))
    if np.ndim(m.pore_volume) != 1:
        raise ValueError("transport: volumes must be one per element")
    validate(m)
    return m


def _structure(mesh) -> Structure:
    s = getattr(mesh, "_structure", None)
    if s is None:
        s = validate(mesh)
        mesh._structure = s
    return s


def check_params(t_end, cfl, nreport=1, max_steps=0):
    if not t_end > 0 or not np.isfinite(t_end):
        raise ValueError("transport: t_end must be positive")
    if not (0 < cfl <= 1):
        raise ValueError("transport: cfl outside (0, 1]")
    if not (1 <= nreport <= 4096):
        raise ValueError("transport: nreport outside [1, 4096]")
    if not (0 <= max_steps <= 2 ** 24):
        raise ValueError("transport: max_steps outside [0, 2^24]")
    return max_steps if max_steps else DEFAULT_MAX_STEPS


def _rates(s: Structure, V, u, dtype):
    """g (n_elem, width) and r_e of one realization, rate"""
    uf = np.asarray(u, dtype)[s.face]
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.where(s.mask, s.sign.astype(dtype) * (s.a.astype(dtype)[s.face] * uf), dtype(0))
        out = np.zeros(len(V), dtype)
        inn = np.zeros(len(V), dtype)
        for l in range(s.width):
            out = out + np.maximum(g[:, l], 0)
            inn = inn + np.maximum(-g[:, l], 0)
        r = np.maximum(out, inn)
        q = r / V
        q = np.where(np.isfinite(g).all(axis=1) & np.isfinite(q), q, dtype(np.inf))
    return g, r, q.max()


def _plan_col(rate, t_end, cfl, max_steps, dtype):
    if not np.isfinite(rate):
        return dict(rate=rate, x=dtype(np.inf), nsteps=0, dt=dtype(0), t_reached=dtype(0), status=BAD_FLUX, margin=np.inf)
    x = (dtype(t_end) * rate) / dtype(cfl)
    n = max(1, int(np.ceil(x)))
    near = max(float(np.rint(x)), 1.0)
    margin = float(abs(x - near) / max(x, 1))
    if n > max_steps:
        dt = dtype(cfl) / rate
        return dict(rate=rate, x=x, nsteps=max_steps, dt=dt, t_reached=dtype(max_steps) * dt, status=STEP_LIMIT, margin=margin)
    return dict(rate=rate, x=x, nsteps=n, dt=dtype(t_end) / dtype(n), t_reached=dtype(t_end), status=OK, margin=margin)


def _stack(cols):
    return {k: np.array([c[k] for c in cols]) for k in cols[0]}


def plan(mesh: TransportMesh, u, t_end, cfl, max_steps=0, dtype=np.float64):
    """Per realization (u: (nbatch, >= n_face) or one row): rate, x, nsteps, dt, t_reached, status and the margin of ceil."""
    max_steps = check_params(t_end, cfl, 1, max_steps)
    s = _structure(mesh)
    V = np.asarray(mesh.pore_volume, dtype)
    return _stack([_plan_col(_rates(s, V, row, dtype)[2], t_end, cfl, max_steps, dtype) for row in np.atleast_2d(u)])


def tree_sum(v):
    """the sum of the device's reductions: thread t of 256 adds the entries t, t + 256, ... in ascending order, a butterfly
    over each wave of 64, the four wave sums in ascending order"""
    v = np.asarray(v)
    n = -(-max(len(v), 1) // _THREADS) * _THREADS
    rows = np.zeros(n, v.dtype)
    rows[:len(v)] = v
    acc = np.zeros(_THREADS, v.dtype)
    for chunk in rows.reshape(-1, _THREADS):
        acc = acc + chunk
    lane = np.arange(_THREADS)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lane ^ off]
    total = acc[0]
    for w in range(1, _THREADS // 64):
        total = total + acc[64 * w]
    return total


def report_steps(nsteps, nreport):
    """n_r and the fraction of a step tau_r / dt = (r nsteps - n_r nreport) / nreport, r = 1 .. nreport"""
    r = np.arange(1, nreport + 1, dtype=np.int64)
    n_r = np.minimum(nsteps - 1, (r * nsteps) // nreport)
    return n_r, r * nsteps - n_r * nreport


def advance(mesh: TransportMesh, u, t_end, cfl, nreport=1, max_steps=0, dtype=np.float64):
    """The twin of pmc_transport_run: dict of c (nbatch, n_elem), curve (nbatch, nreport), stored (nbatch,) and the plan's
    entries."""
    max_steps = check_params(t_end, cfl, nreport, max_steps)
    s = _structure(mesh)
    V = np.asarray(mesh.pore_volume, dtype)
    wgt, cin = s.weight.astype(dtype), s.c_in.astype(dtype)
    cols = []
    for row in np.atleast_2d(u):
        g, r, rate = _rates(s, V, row, dtype)
        p = _plan_col(rate, t_end, cfl, max_steps, dtype)
        c = s.c0.astype(dtype)
        curve = np.zeros(nreport, dtype)
        if p["status"] != BAD_FLUX:
            n, dt = p["nsteps"], p["dt"]
            w = dt / V
            d = 1 - w * r
            gin = np.maximum(-g, 0)
            gout = np.maximum(g[s.out_elem, s.out_slot], 0)
            acc = np.zeros(len(s.out_face), dtype)
            n_r, num = report_steps(n, nreport)
            for step in range(n):
                m = gout * c[s.out_elem]
                for i in np.flatnonzero(n_r == step):
                    tau = (dtype(num[i]) / dtype(nreport)) * dt
                    curve[i] = tree_sum(acc + tau * m)
                acc = acc + dt * m
                cn = np.where(s.nbr >= 0, c[s.nbr], cin[s.face])
                sacc = np.zeros(len(V), dtype)
                for l in range(s.width):
                    sacc = sacc + gin[:, l] * cn[:, l]
                c = d * c + w * sacc
        cols.append(dict(p, c=c, curve=curve, stored=tree_sum(wgt * c)))
    return _stack(cols)


def inflow_mass_rate(mesh: TransportMesh, u, dtype=np.float64):
    """sum over boundary dofs of max(-g, 0) c_in per realization: the solute mass entering per unit time"""
    s = _structure(mesh)
    V = np.asarray(mesh.pore_volume, dtype)
    out = []
    for row in np.atleast_2d(u):
        g = _rates(s, V, row, dtype)[0]
        bd = s.mask & (s.nbr < 0)
        out.append((np.maximum(-g, 0) * s.c_in.astype(dtype)[s.face])[bd].sum())
    return np.array(out)


def reduce(curve, stored, kind=MASS_OUT):
    """Q per realization: the mass that left through the outlet by t_reached (MASS_OUT) or the weighted mass in place (STORED)"""
    if kind not in (MASS_OUT, STORED):
        raise ValueError("transport: kind must be MASS_OUT or STORED")
    return np.atleast_2d(curve)[:, -1].copy() if kind == MASS_OUT else np.atleast_1d(stored).copy()


# ---- the discrete adjoint (csrc/transport.hip, pmc_transport_run_adjoint) -------------------------------
# Three decisions of the forward pass are held fixed: the step count, the sign of every g (strictly positive, strictly
# negative, or zero: nothing) and the branch sigma_e = (out_e >= in_e) of r_e.  Under them the scheme is a polynomial in u.
def _sides(s: Structure):
    """per dof the (element, row slot) of its one or two entries, ascending element; second element -1 on a boundary dof"""
    t = getattr(s, "_sides", None)
    if t is None:
        e, l = np.nonzero(s.mask)
        f = s.face[e, l]
        order = np.lexsort((e, f))
        e, l, f = e[order], l[order], f[order]
        start = np.flatnonzero(np.concatenate([[True], f[1:] != f[:-1]]))
        two = np.concatenate([f[1:] == f[:-1], [False]])[start]
        second = np.where(two, np.minimum(start + 1, len(f) - 1), start)
        oidx = np.full(s.face.shape, -1, np.int64)
        oidx[s.out_elem, s.out_slot] = np.arange(len(s.out_face))
        t = (e[start], l[start], np.where(two, e[second], -1), l[second], oidx)
        s._sides = t
    return t


def _setup_col(s, V, row, t_end, cfl, max_steps, dtype, dec):
    """rates, decisions and step sizes of one column; dec: (nsteps, sign(g), sigma) to be taken as they are"""
    g, r, rate = _rates(s, V, row, dtype)
    if dec is None:
        p = _plan_col(rate, t_end, cfl, max_steps, dtype)
        if p["status"] != OK:
            return p, None
        sgn = np.sign(g).astype(np.int8)
    else:
        n = int(dec[0])
        p = dict(rate=rate, x=(dtype(t_end) * rate) / dtype(cfl), nsteps=n, dt=dtype(t_end) / dtype(n), t_reached=dtype(t_end),
                 status=OK, margin=np.inf)
        sgn = np.asarray(dec[1], np.int8)
    go = np.where(sgn > 0, g, dtype(0))
    gi = np.where(sgn < 0, -g, dtype(0))
    out = np.zeros(len(V), dtype)
    inn = np.zeros(len(V), dtype)
    for l in range(s.width):
        out = out + go[:, l]
        inn = inn + gi[:, l]
    sigma = (out >= inn) if dec is None else np.asarray(dec[2], bool)
    w = p["dt"] / V
    nz = np.abs(g[sgn != 0]).astype(np.float64)
    return p, dict(g=g, sgn=sgn, go=go, gi=gi, sigma=sigma, tied=out == inn, w=w, d=1 - w * np.where(sigma, out, inn),
                   g_margin=float(nz.min() / nz.max()) if nz.size else np.inf)


def _step(s, q, cin, c):
    cn = np.where(s.nbr >= 0, c[s.nbr], cin[s.face])
    sacc = np.zeros(len(c), c.dtype)
    for l in range(s.width):
        sacc = sacc + q["gi"][:, l] * cn[:, l]
    return q["d"] * c + q["w"] * sacc


def _forward_col(s, q, p, wgt, cin, nreport, dtype, keep):
    """the forward pass of advance under the decisions; keep(n, c) is handed every state c^n, n = 0 .. nsteps - 1"""
    n, dt = p["nsteps"], p["dt"]
    c = s.c0.astype(dtype)
    curve = np.zeros(nreport, dtype)
    gout = q["go"][s.out_elem, s.out_slot]
    acc = np.zeros(len(s.out_face), dtype)
    n_r, num = report_steps(n, nreport)
    for step in range(n):
        keep(step, c)
        m = gout * c[s.out_elem]
        for i in np.flatnonzero(n_r == step):
            curve[i] = tree_sum(acc + ((dtype(num[i]) / dtype(nreport)) * dt) * m)
        acc = acc + dt * m
        c = _step(s, q, cin, c)
    return c, curve, tree_sum(wgt * c)


class _History:
    """c^n for n < nsteps: all of them (segment None), or every segment-th one with the states between recomputed a segment
    at a time by the forward step - the device's scheme; the recomputed bits are the forward bits"""

    def __init__(self, s, q, cin, segment):
        self.s, self.q, self.cin, self.K = s, q, cin, segment
        self.kept, self.seg, self.seg_of = {}, [], -1

    def keep(self, n, c):
        if self.K is None or n % self.K == 0:
            self.kept[n] = c

    def __call__(self, n):
        if self.K is None:
            return self.kept[n]
        i = n // self.K
        if i != self.seg_of:
            self.seg = [self.kept[i * self.K]]
            for _ in range(self.K - 1):
                self.seg.append(_step(self.s, self.q, self.cin, self.seg[-1]))
            self.seg_of = i
        return self.seg[n - i * self.K]


def _seed(x, shape, what, dtype):
    if x is None:
        return None
    x = np.asarray(x, dtype)
    if x.shape != shape:
        raise ValueError(f"transport: {what} must have the shape {shape}")
    return x


def _check_adjoint(mesh, u, t_end, cfl, nreport, max_steps, curve_bar, stored_bar, c_bar, dtype, segment, decisions):
    max_steps = check_params(t_end, cfl, nreport, max_steps)
    if u is None:
        raise ValueError("transport: u is missing")
    u = np.atleast_2d(u)
    nb = len(u)
    if u.shape[1] < mesh.n_face:
        raise ValueError("transport: a row of u is shorter than the number of flux dofs")
    if curve_bar is None and stored_bar is None and c_bar is None:
        raise ValueError("transport: at least one of curve_bar, stored_bar and c_bar must be given")
    if segment is not None and segment < 1:
        raise ValueError("transport: the segment length must be at least 1")
    if decisions is not None and len(decisions) != nb:
        raise ValueError("transport: one set of decisions per column")
    cb = _seed(None if curve_bar is None else np.atleast_2d(curve_bar), (nb, nreport), "curve_bar", dtype)
    sb = _seed(None if stored_bar is None else np.atleast_1d(stored_bar), (nb,), "stored_bar", dtype)
    eb = _seed(None if c_bar is None else np.atleast_2d(c_bar), (nb, mesh.n_elem), "c_bar", dtype)
    return max_steps, u, cb, sb, eb


def advance_adjoint(mesh: TransportMesh, u, t_end, cfl, nreport, curve_bar=None, stored_bar=None, c_bar=None, max_steps=0,
                    dtype=np.float64, decisions=None, segment=None):
    """The twin of pmc_transport_run_adjoint: for J = <curve_bar, curve> + stored_bar stored + <c_bar, c> per column the
    gradients u_bar (nbatch, n_face) in the flux and c0_bar (nbatch, n_elem) in the initial concentration, beside the forward
    results of advance.  Also returns `decisions`, per column (nsteps, sign(g), sigma) or None where the status is not OK (such
    a column has zero gradients), `tied` (the elements with out_e == in_e) and `g_margin`, the smallest |g| / max |g| over the
    nonzero g.  decisions=: take these instead of deciding (an np.longdouble run on the float64 run's decisions).  segment=:
    keep every segment-th state and recompute the others, as the device does; the bits do not depend on it."""
    max_steps, u, cbs, sbs, ebs = _check_adjoint(mesh, u, t_end, cfl, nreport, max_steps, curve_bar, stored_bar, c_bar, dtype,
                                                 segment, decisions)
    s = _structure(mesh)
    e1, l1, e2, l2, oidx = _sides(s)
    V = np.asarray(mesh.pore_volume, dtype)
    wgt, cin, a = s.weight.astype(dtype), s.c_in.astype(dtype), s.a.astype(dtype)
    ne, nf = len(V), len(a)
    interior, outl = s.nbr >= 0, oidx >= 0
    cols, decs = [], []
    for b, row in enumerate(u):
        dec = None if decisions is None else decisions[b]
        p, q = (_setup_col(s, V, row, t_end, cfl, max_steps, dtype, dec) if decisions is None or dec is not None
                else (_plan_col(_rates(s, V, row, dtype)[2], t_end, cfl, max_steps, dtype), None))
        if q is None:
            f = advance(mesh, row, t_end, cfl, nreport, max_steps, dtype)
            cols.append(dict(p, c=f["c"][0], curve=f["curve"][0], stored=f["stored"][0], u_bar=np.zeros(nf, dtype),
                             c0_bar=np.zeros(ne, dtype), g_margin=np.inf, tied=np.zeros(ne, bool)))
            decs.append(None)
            continue
        n, dt, w, d, sgn, go = p["nsteps"], p["dt"], q["w"], q["d"], q["sgn"], q["go"]
        hist = _History(s, q, cin, segment)
        c, curve, stored = _forward_col(s, q, p, wgt, cin, nreport, dtype, hist.keep)
        cb = np.zeros(nreport, dtype) if cbs is None else cbs[b]
        n_r, num = report_steps(n, nreport)
        lam = (dtype(0) if sbs is None else sbs[b]) * wgt + (np.zeros(ne, dtype) if ebs is None else ebs[b])
        P = np.zeros(ne, dtype)
        X = np.zeros(s.face.shape, dtype)
        O = np.zeros(len(s.out_face), dtype)
        for step in range(n - 1, -1, -1):
            s1 = dtype(0)
            for i in np.flatnonzero(n_r > step):
                s1 = s1 + cb[i]
            beta = dt * s1
            for i in np.flatnonzero(n_r == step):
                beta = beta + ((dtype(num[i]) / dtype(nreport)) * dt) * cb[i]
            cn_ = hist(step)
            wl = w * lam
            y = np.where(interior, wl[s.nbr], np.where(outl, beta, dtype(0)))
            sacc = np.zeros(ne, dtype)
            for l in range(s.width):
                sacc = sacc + go[:, l] * y[:, l]
            cn = np.where(interior, cn_[s.nbr], cin[s.face])
            X = X + np.where(sgn < 0, cn * lam[:, None], dtype(0))
            O = O + beta * cn_[s.out_elem]
            P = P + cn_ * lam
            lam = d * lam + sacc
        t1 = (w * P)[:, None]
        sig = q["sigma"][:, None]
        G = np.where((sgn > 0) & sig, -t1, np.where((sgn < 0) & ~sig, t1, dtype(0)))
        G = np.where(sgn < 0, G - w[:, None] * X, G)
        G = np.where(outl & (sgn > 0), G + O[np.maximum(oidx, 0)], G)
        G = s.sign.astype(dtype) * G
        acc = np.zeros(nf, dtype) + G[e1, l1]
        acc = np.where(e2 >= 0, acc + G[np.maximum(e2, 0), l2], acc)
        cols.append(dict(p, c=c, curve=curve, stored=stored, u_bar=a * acc, c0_bar=lam, g_margin=q["g_margin"], tied=q["tied"]))
        decs.append((n, sgn, q["sigma"]))
    out = _stack(cols)
    out["decisions"] = decs
    return out


def advance_tangent(mesh: TransportMesh, u, du, t_end, cfl, nreport, max_steps=0, dtype=np.float64, decisions=None):
    """The linearisation of advance in u under the decisions of advance_adjoint: dict of dcurve (nbatch, nreport), dstored
    (nbatch,), dc (nbatch, n_elem) for the directions du (nbatch, >= n_face); zero where the status is not OK.  numpy only."""
    max_steps = check_params(t_end, cfl, nreport, max_steps)
    if u is None or du is None:
        raise ValueError("transport: u or du is missing")
    u, du = np.atleast_2d(u), np.atleast_2d(du)
    if u.shape[1] < mesh.n_face or du.shape[1] < mesh.n_face or len(u) != len(du):
        raise ValueError("transport: u and du must have the same number of rows of at least n_face entries")
    s = _structure(mesh)
    V = np.asarray(mesh.pore_volume, dtype)
    wgt, cin, a = s.weight.astype(dtype), s.c_in.astype(dtype), s.a.astype(dtype)
    cols = []
    for b, row in enumerate(u):
        p, q = _setup_col(s, V, row, t_end, cfl, max_steps, dtype, None if decisions is None else decisions[b])
        if q is None:
            cols.append(dict(dcurve=np.zeros(nreport, dtype), dstored=dtype(0), dc=np.zeros(len(V), dtype)))
            continue
        n, dt, w, d, sgn = p["nsteps"], p["dt"], q["w"], q["d"], q["sgn"]
        dg = np.where(s.mask, s.sign.astype(dtype) * (a[s.face] * np.asarray(du[b], dtype)[s.face]), dtype(0))
        dgo, dgi = np.where(sgn > 0, dg, dtype(0)), np.where(sgn < 0, -dg, dtype(0))
        dd = -w * np.where(q["sigma"], dgo.sum(axis=1), dgi.sum(axis=1))
        gout, dgout = q["go"][s.out_elem, s.out_slot], dgo[s.out_elem, s.out_slot]
        c, dc = s.c0.astype(dtype), np.zeros(len(V), dtype)
        acc, dacc = np.zeros(len(s.out_face), dtype), np.zeros(len(s.out_face), dtype)
        dcurve = np.zeros(nreport, dtype)
        n_r, num = report_steps(n, nreport)
        for step in range(n):
            dm = dgout * c[s.out_elem] + gout * dc[s.out_elem]
            for i in np.flatnonzero(n_r == step):
                dcurve[i] = (dacc + ((dtype(num[i]) / dtype(nreport)) * dt) * dm).sum()
            dacc = dacc + dt * dm
            cn = np.where(s.nbr >= 0, c[s.nbr], cin[s.face])
            dcn = np.where(s.nbr >= 0, dc[s.nbr], dtype(0))
            dc = dd * c + d * dc + w * (dgi * cn + q["gi"] * dcn).sum(axis=1)
            c = _step(s, q, cin, c)
        cols.append(dict(dcurve=dcurve, dstored=(wgt * dc).sum(), dc=dc))
    return _stack(cols)
