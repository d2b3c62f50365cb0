"""MixMaterial of the pure-Python float32 restatement (test infrastructure), on top of tests/refpy_bsdf_full.py, from
the reference text, NOT from the HIP:
* ScaledBxDF (src/core/reflection.h:225-245, reflection.cpp:97-110): f and Sample_f are scale * the inner lobe's, per
  channel in float; Pdf and the type are the inner lobe's;
* MixMaterial::ComputeScatteringFunctions (src/materials/mixmat.cpp:46-64): s1 = amount.Clamp(),
  s2 = (Spectrum(1.f) - s1).Clamp(), the first child's BxDFs wrapped under s1 in order, then the second's under s2.
  A ScaledBxDF is added even where its scale is black: it counts in NumComponents, takes its share of
  floor(u0 * n) and divides the pdf.  A nest wraps again: s_outer * (s_inner * f);
* the two lobes a mirror or a smooth glass brings to a mix (both walks pass allowMultipleLobes = true,
  photonbeam.cpp:298, 514): SpecularReflection under FresnelNoOp (mirror.cpp:50-56, reflection.cpp:136-143) and
  FresnelSpecular (glass.cpp:71-73, reflection.cpp:477-511), which sets the sampled type itself;
* BSDF::Sample_f's sampledType (reflection.cpp:737-738): the lobe's type unless the lobe's Sample_f changes it.
A table is a list of scene.MaterialEx whose mixes name earlier entries (scene.mix).

`stats` counts, besides refpy_bsdf_full's counters, the branches a mix brings (COUNTERS).
"""
from __future__ import annotations

import math

import numpy as np

import refpy_bsdf as rb
import refpy_bsdf_full as rf
from refpy_bsdf import _clamp01, _count
from refpy_bsdf_full import (BSDF_ALL, BSDF_REFLECTION, BSDF_SPECULAR, BSDF_TRANSMISSION, IMPORTANCE, RADIANCE, ZERO3,
                             _abs, _black)
from refpy_photon import ONE_MINUS_EPS, dot, f32
from refpy_specular import fr_dielectric, refract, to_world

MIRROR, GLASS, INTERFACE, MIX = 1, 2, 3, 12
MAX_MIX_DEPTH, MAX_BXDFS = 4, 8

MIX_COUNTERS = ("chosen_spec_noop", "chosen_fresnel_spec", "fresnel_spec_reflect", "fresnel_spec_transmit",
                "zero_scale_sampled", "specular_of_both", "nonspecular_of_both", "chain_depth2", "chain_depth3",
                "lobes6", "lobes7", "lobes8")
COUNTERS = rf.COUNTERS + MIX_COUNTERS


def new_stats():
    return {k: 0 for k in COUNTERS}


def sample_t(b, wo, u0, u1, mode, stats=None, normals=None):
    """A lobe's Sample_f with the sampled type: (wi, pdf, f, type); the type is the lobe's unless it sets it."""
    if hasattr(b, "sample_t"):
        return b.sample_t(wo, u0, u1, mode, stats, normals)
    return b.sample(wo, u0, u1, mode, stats, normals) + (b.type,)


class SpecularNoOp:
    """SpecularReflection(R, FresnelNoOp): fresnel->Evaluate is Spectrum(1.)."""
    type = BSDF_REFLECTION | BSDF_SPECULAR
    key = "chosen_spec_noop"

    def __init__(self, R):
        self.R = R

    def f(self, wo, wi, mode):
        return ZERO3

    def pdf(self, wo, wi):
        return f32(0)

    def sample(self, wo, u0, u1, mode, stats=None, normals=None):
        wi = (-wo[0], -wo[1], wo[2])
        ac = _abs(wi[2])
        with np.errstate(all="ignore"):
            return wi, f32(1), tuple(f32(f32(f32(1) * r) / ac) for r in self.R)


class FresnelSpecular:
    type = BSDF_REFLECTION | BSDF_TRANSMISSION | BSDF_SPECULAR
    key = "chosen_fresnel_spec"

    def __init__(self, R, T, eta_a, eta_b):
        self.R, self.T, self.eta_a, self.eta_b = R, T, f32(eta_a), f32(eta_b)

    def f(self, wo, wi, mode):
        return ZERO3

    def pdf(self, wo, wi):
        return f32(0)

    def sample_t(self, wo, u0, u1, mode, stats=None, normals=None):
        F, _ = fr_dielectric(wo[2], self.eta_a, self.eta_b)
        if u0 < F:
            _count(stats, "fresnel_spec_reflect")
            wi = (-wo[0], -wo[1], wo[2])
            ac = _abs(wi[2])
            with np.errstate(all="ignore"):
                return wi, F, tuple(f32(f32(F * r) / ac) for r in self.R), BSDF_SPECULAR | BSDF_REFLECTION
        entering = wo[2] > 0
        eta_i, eta_t = (self.eta_a, self.eta_b) if entering else (self.eta_b, self.eta_a)
        n = (f32(-0.0), f32(-0.0), f32(-1)) if wo[2] < 0 else (f32(0), f32(0), f32(1))  # Faceforward(Normal3f(0,0,1), wo)
        wi = refract(wo, n, f32(eta_i / eta_t))
        if wi is None:
            return ZERO3, f32(0), ZERO3, self.type
        _count(stats, "fresnel_spec_transmit")
        out = []
        ac = _abs(wi[2])
        for t in self.T:
            ft = f32(t * f32(f32(1) - F))
            if mode == RADIANCE:
                ft = f32(ft * f32(f32(eta_i * eta_i) / f32(eta_t * eta_t)))
            with np.errstate(all="ignore"):
                out.append(f32(ft / ac))
        return wi, f32(f32(1) - F), tuple(out), BSDF_SPECULAR | BSDF_TRANSMISSION

    def sample(self, wo, u0, u1, mode, stats=None, normals=None):
        return self.sample_t(wo, u0, u1, mode, stats, normals)[:3]


class GlossyLobe:
    """One lobe of a refpy_bsdf.Bsdf (matte, plastic, metal) behind refpy_bsdf_full's lobe convention."""

    def __init__(self, b, lobe):
        self.b, self.lobe = b, lobe
        self.type = b.lobe_type(lobe)
        self.key = "chosen_micro_r" if lobe == rb.MICRO else "chosen_lambert_r"

    def f(self, wo, wi, mode):
        return self.b.lobe_f(self.lobe, wo, wi)

    def pdf(self, wo, wi):
        return self.b.lobe_pdf(self.lobe, wo, wi)

    def sample(self, wo, u0, u1, mode, stats=None, normals=None):
        return self.b.lobe_sample(self.lobe, wo, u0, u1, stats, normals)


class ScaledBxDF:
    def __init__(self, bxdf, scale):
        self.bxdf, self.scale = bxdf, tuple(f32(x) for x in scale)
        self.type, self.key = bxdf.type, bxdf.key
        self.depth = getattr(bxdf, "depth", 0) + 1  # enclosing mixes

    def _scaled(self, f):
        with np.errstate(all="ignore"):
            return tuple(f32(s * x) for s, x in zip(self.scale, f))

    def f(self, wo, wi, mode):
        return self._scaled(self.bxdf.f(wo, wi, mode))

    def pdf(self, wo, wi):
        return self.bxdf.pdf(wo, wi)

    def sample_t(self, wo, u0, u1, mode, stats=None, normals=None):
        wi, pdf, f, typ = sample_t(self.bxdf, wo, u0, u1, mode, stats, normals)
        return wi, pdf, self._scaled(f), typ

    def sample(self, wo, u0, u1, mode, stats=None, normals=None):
        return self.sample_t(wo, u0, u1, mode, stats, normals)[:3]

    def zero_scale(self):
        return _black(self.scale) or getattr(self.bxdf, "zero_scale", lambda: False)()


def lobes_of(table, k):
    """The BxDFs entry k's ComputeScatteringFunctions adds, in order."""
    m = table[k]
    if m.type == MIX:
        s1 = tuple(_clamp01(x) for x in m.amount)
        s2 = tuple(rf._max(f32(f32(1) - x), f32(0)) for x in s1)
        c1, c2 = m.mix_child[0], m.mix_child[1]
        assert 0 <= c1 < k and 0 <= c2 < k, "a mix's children come earlier in the table"
        return [ScaledBxDF(b, s1) for b in lobes_of(table, c1)] + [ScaledBxDF(b, s2) for b in lobes_of(table, c2)]
    if m.type == MIRROR:
        R = tuple(_clamp01(x) for x in m.kr)
        return [] if _black(R) else [SpecularNoOp(R)]
    if m.type == GLASS:
        R, T = tuple(_clamp01(x) for x in m.kr), tuple(_clamp01(x) for x in m.kt)
        return [] if _black(R) and _black(T) else [FresnelSpecular(R, T, 1, m.eta)]
    assert m.type != INTERFACE, "an interface has no BSDF to scale"
    if m.type >= rf.ROUGH_GLASS:
        return list(rf.FullBsdf.of(m).lobes)
    b = rb.Bsdf.of(m)
    return [GlossyLobe(b, lobe) for lobe in b.lobes]


class MixBsdf(rf.FullBsdf):
    """The BSDF a MixMaterial leaves: FullBsdf's f, Pdf and matching over ScaledBxDFs, and BSDF::Sample_f once more
    for the sampled type and the counters."""

    def __init__(self, lobes):
        self.kind = MIX
        self.lobes = list(lobes)
        assert len(self.lobes) <= MAX_BXDFS, "BSDF::Add CHECK_LTs against MaxBxDFs (reflection.h:166)"
        self.none = not self.lobes

    def sample(self, q, wo_w, u0, u1, flags=BSDF_ALL, mode=RADIANCE, stats=None, normals=None):
        match = self.matching(flags)
        n = len(match)
        if n == 0:
            _count(stats, "no_matching_lobe")
            return None
        u0, u1 = f32(u0), f32(u1)
        comp = min(int(math.floor(f32(u0 * f32(n)))), n - 1)
        b = match[comp]
        ur = f32(f32(u0 * f32(n)) - f32(comp))
        ur = ur if ur < ONE_MINUS_EPS else ONE_MINUS_EPS
        wo = rb._to_local(q, wo_w)
        if wo[2] == 0:
            return None
        _count(stats, b.key)
        if b.zero_scale():
            _count(stats, "zero_scale_sampled")
        if b.depth in (2, 3):
            _count(stats, "chain_depth%d" % b.depth)
        if n in (6, 7, 8):
            _count(stats, "lobes%d" % n)
        wi, pdf, f, typ = sample_t(b, wo, ur, u1, mode, stats, normals)  # *sampledType = bxdf->type, then Sample_f
        if pdf == 0:
            return None
        wi_w = to_world(q, wi)
        specular = bool(b.type & BSDF_SPECULAR)
        if len({bool(x.type & BSDF_SPECULAR) for x in match}) == 2:
            _count(stats, "specular_of_both" if specular else "nonspecular_of_both")
        with np.errstate(all="ignore"):
            if not specular and n > 1:
                for other in match:
                    if other is not b:
                        pdf = f32(pdf + other.pdf(wo, wi))
            if n > 1:
                pdf = f32(pdf / f32(n))
            if not specular and n > 1:
                reflect = f32(dot(wi_w, q["n"]) * dot(wo_w, q["n"])) > 0
                f = self._sum_f(match, reflect, wo, wi, mode)
        return wi_w, pdf, f, typ


def bsdf_of(table, k):
    """The restated BSDF of entry k (type >= 4) of `table`, behind refpy_bsdf_full.bsdf_of's calling convention."""
    m = table[k]
    return MixBsdf(lobes_of(table, k)) if m.type == MIX else rf.bsdf_of(m)
