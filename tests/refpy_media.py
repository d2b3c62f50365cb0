"""A medium of the pure-Python float32 restatement (test infrastructure): HomogeneousMedium
(src/media/homogeneous.cpp) or GridDensityMedium (src/media/grid.cpp, restated in refpy_photon), and the two
calls the passes make on the medium a ray carries.  A ray in vacuum (a null Medium*, here None) draws nothing
and has Tr = 1.  Every float operation is done on numpy float32 scalars in the reference's order.
"""
from __future__ import annotations

import ctypes

import numpy as np

from refpy_photon import MAXF, expf, f32, grid_sample, grid_tr, length, logf

HOMOGENEOUS, GRID = 1, 2
ONE3 = (f32(1),) * 3


class Medium:
    """A bre_medium as the HomogeneousMedium / GridDensityMedium constructors see it (the attribute names are
    those refpy_photon's grid functions read).  A bre_scene's own medium has the same fields under the same
    names, its kind in has_medium: Medium(scene, scene.has_medium)."""

    def __init__(self, m, kind=None):
        self.grid = int(m.type if kind is None else kind) == GRID
        self.sigma_t = tuple(f32(f32(a) + f32(b)) for a, b in zip(m.sigma_a, m.sigma_s))
        self.g = f32(m.g)
        if self.grid:  # grid.h:58-77
            self.n = tuple(int(v) for v in m.grid_n)
            self.m = [[f32(m.world_to_medium[4 * i + j]) for j in range(4)] for i in range(4)]
            cnt = self.n[0] * self.n[1] * self.n[2]
            self.density = np.ctypeslib.as_array((ctypes.c_float * cnt).from_address(m.grid_density)).copy()
            self.gsig = self.sigma_t[0]
            mx = f32(0)
            for v in self.density:
                mx = v if mx < v else mx
            self.inv_max = f32(f32(1) / mx)

    def tr(self, d, tmax):  # HomogeneousMedium::Tr, homogeneous.cpp:44-48
        x = f32(tmax * length(d))
        x = MAXF if MAXF < x else x
        return tuple(expf(f32(f32(-st) * x)) for st in self.sigma_t)


def med_sample(M, rng, o, d, tmax):
    """Medium::Sample's distance decision: the t of the interaction, or None (None at once in vacuum)."""
    if M is None:
        return None
    if M.grid:
        return grid_sample(M, rng, o, d, tmax)
    ch = min(int(f32(rng.uniform() * f32(3))), 2)
    dist = f32(-logf(f32(f32(1) - rng.uniform())) / M.sigma_t[ch])
    dl = f32(dist * length(d))
    t = tmax if tmax < dl else dl
    return t if t < tmax else None


def med_tr(M, smp, o, d, tmax):
    if M is None:
        return ONE3
    if M.grid:
        return (grid_tr(M, smp, o, d, tmax),) * 3
    return M.tr(d, tmax)
