"""Setup side of the sampler drivers' result table (examples/PDESamplerTest.cpp:186-192): the indicator chi of the element
nearest the centre of mass, restricted level by level with P^T.  The statistics themselves run on the device
(capi.FieldStatistics)."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np


def _seq_sum(a: np.ndarray) -> float:
    """left-to-right sum (the reference's serial InnerProduct loop), not numpy's pairwise one"""
    return float(np.cumsum(a)[-1]) if a.size else 0.0


def chi_center_of_mass(space) -> np.ndarray:
    """chi_center_of_mass (src/Utilities.cpp:340-395): 1 on the element whose P0 projection of the coordinates lies nearest
    the volume-weighted centre of mass, 0 elsewhere.  ProjectCoefficient of x on L2 P0 evaluates x at the element's
    reference centre: the vertex mean on straight-sided simplices, quadrilaterals and hexahedra.  Ties keep the first
    element (`<`, :385)."""
    m = space.mesh
    vol = np.asarray(space.vol, np.float64)
    xe = m.verts[m.elems].mean(axis=1)                  # (ne, dim)
    volume = _seq_sum(vol)
    cm = np.array([_seq_sum(vol * xe[:, d]) / volume for d in range(m.dim)])
    dist2 = np.zeros(m.ne)
    for d in range(m.dim):
        dd = cm[d] - xe[:, d]
        dist2 = dist2 + dd * dd
    dist = np.sqrt(dist2)
    chi = np.zeros(m.ne)
    chi[int(np.argmin(dist))] = 1.0                     # first minimum, like the strict `<` of the reference
    return chi


def restrict_chi(chi0: np.ndarray, P: Sequence) -> List[np.ndarray]:
    """[chi_0, P_0^T chi_0, P_1^T P_0^T chi_0, ...] (PDESamplerTest.cpp:186-192: GetTrueP(l)->MultTranspose)."""
    out = [np.asarray(chi0, np.float64)]
    for Pl in P:
        out.append(np.asarray(Pl.T @ out[-1], np.float64))
    return out
