"""The two walks over surfaces under a MixMaterial (test infrastructure), on top of tests/refpy_passes_full.py without
editing it, from the reference text, NOT from the HIP.

Neither walk knows a mix: photonbeam.cpp:296-323 and :512-554 call BSDF::Sample_f(..., BSDF_ALL) on whatever BSDF the
material left, and EstimateDirect sees it under BSDF_ALL & ~BSDF_SPECULAR (integrator.cpp:112-113).  So the walks are
refpy_passes_full's own, over a Scene whose mix entries hold tests/refpy_mix.py's MixBsdf: the sampled type, which the
camera walk's specularBounce reads (:543), is the one the chosen lobe reports (FresnelSpecular sets its own).
A beam's tag is refpy_passes_full's: the BxDFType bits of the surface bounce that spawned its ray, for the triangles
under a mix as for those under a rough glass, uber, translucent or substrate.
"""
from __future__ import annotations

import refpy_bsdf as rb
import refpy_mix as rm
import refpy_passes_full as rpf

COUNTERS = rpf.COUNTERS + rm.MIX_COUNTERS
trace_photons, camera_pass = rpf.trace_photons, rpf.camera_pass


def new_stats():
    return {k: 0 for k in COUNTERS}


class Scene(rpf.Scene):
    """refpy_passes_full.Scene whose table may hold mixes (the classes below it see a matte in their place);
    self.mixed: the triangles under one."""

    def __init__(self, s, lights=(), materials=(), triangle_material=(), *media_args, **kw):
        materials = list(materials)
        stand_in = []
        for m in materials:
            if m.type == rm.MIX:
                p = type(m)()
                p.type = rb.MATTE
                p.kd[0] = p.kd[1] = p.kd[2] = 0.5
                stand_in.append(p)
            else:
                stand_in.append(m)
        super().__init__(s, lights, stand_in, triangle_material, *media_args, **kw)
        table = {k: rpf.LobedBsdf(rm.bsdf_of(materials, k), False) for k, m in enumerate(materials) if m.type == rm.MIX}
        self.mixed = set()
        for i, k in enumerate(triangle_material if materials else ()):
            if k in table:
                self.bsdf[i] = table[k]
                self.lobed.add(i)
                self.mixed.add(i)
