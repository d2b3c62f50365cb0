"""The BSDF of any number of lobes of the pure-Python float32 restatement (test infrastructure), with BxDFType flags
and a TransportMode, and the materials that need it, each from the reference text, NOT from the HIP:
* the materials: GlassMaterial::ComputeScatteringFunctions with a roughness (src/materials/glass.cpp:45-92),
  UberMaterial's (src/materials/uber.cpp:45-101), TranslucentMaterial's (src/materials/translucent.cpp:45-80),
  SubstrateMaterial's (src/materials/substrate.cpp:45-65);
* the lobes: SpecularReflection::Sample_f under FresnelDielectric (src/core/reflection.cpp:128-143),
  SpecularTransmission::Sample_f (:150-166), LambertianReflection / LambertianTransmission (:178-190, 378-403),
  MicrofacetReflection (:226-236, 405-423), MicrofacetTransmission (:244-266, 425-448), FresnelBlend (:285-298,
  450-475, SchlickFresnel reflection.h:488-491), with Refract (reflection.h:96-108);
* the BSDF: BxDF::MatchesFlags (reflection.h:218), BSDF::NumComponents (:523-528), BSDF::f (reflection.cpp:670-683),
  BSDF::Pdf (:770-785), BSDF::Sample_f (:703-768).
Every float operation is done on numpy float32 scalars in the reference's order; the one exception is
TrowbridgeReitzSample11's normal-incidence branch, as in tests/refpy_bsdf.py, whose distribution this module uses.
BSDF::eta is read nowhere in photonbeam.cpp and is not kept.

`stats`, a dict from new_stats(), counts the branches taken (COUNTERS); `normals` receives (r, phi) of every
normal-incidence sample.
"""
from __future__ import annotations

import math

import numpy as np

import refpy_bsdf as rb
from refpy_bsdf import _clamp01, _count, _divf, _max, tr_D, tr_G, tr_pdf, tr_sample_wh
from refpy_photon import INV_PI, ONE_MINUS_EPS, PI, add, cosine_hemisphere, dot, f32, mul, normalize
from refpy_specular import IMPORTANCE, RADIANCE, ZERO3, fr_dielectric, refract, to_world

ROUGH_GLASS, UBER, TRANSLUCENT, SUBSTRATE = 8, 9, 10, 11
BSDF_REFLECTION, BSDF_TRANSMISSION, BSDF_DIFFUSE, BSDF_GLOSSY, BSDF_SPECULAR = 1, 2, 4, 8, 16
BSDF_ALL = 31
BSDF_NON_SPECULAR = BSDF_ALL & ~BSDF_SPECULAR

COUNTERS = rb.COUNTERS + (
    "chosen_spec_r", "chosen_spec_t", "chosen_lambert_r", "chosen_lambert_t", "chosen_micro_r", "chosen_micro_t",
    "chosen_blend", "tir_spec_t", "tir_micro_t", "wh_flipped", "blend_diffuse_half", "blend_specular_half",
    "micro_r_other_hemisphere", "blend_other_hemisphere", "sampled_specular_of_mixed", "sampled_nonspecular_of_mixed",
    "no_matching_lobe")


def new_stats():
    return {k: 0 for k in COUNTERS}


def _abs(x):
    return f32(abs(x))


def _pow5(v):
    return f32(f32(f32(v * v) * f32(v * v)) * v)


def _same_hemisphere(w, wp):
    return f32(w[2] * wp[2]) > 0


def _neg(v):
    return tuple(-x for x in v)


def _reflect(wo, n):
    """Reflect, reflection.h:92-94: -wo + 2 * Dot(wo, n) * n."""
    return add(_neg(wo), mul(n, f32(f32(2) * dot(wo, n))))


# ---- the lobes, in the shading frame: type, f(wo, wi, mode), pdf(wo, wi), sample(wo, u0, u1, mode, stats, normals)
# -> (wi, pdf, f) with pdf = 0 where Sample_f returns before it sets *pdf (it arrived as 0) ----
class SpecularReflection:
    type = BSDF_REFLECTION | BSDF_SPECULAR
    key = "chosen_spec_r"

    def __init__(self, R, eta_a, eta_b):
        self.R, self.eta_a, self.eta_b = R, f32(eta_a), f32(eta_b)

    def f(self, wo, wi, mode):
        return ZERO3

    def pdf(self, wo, wi):
        return f32(0)

    def sample(self, wo, u0, u1, mode, stats=None, normals=None):
        wi = (-wo[0], -wo[1], wo[2])
        F, _ = fr_dielectric(wi[2], self.eta_a, self.eta_b)
        ac = _abs(wi[2])
        with np.errstate(all="ignore"):
            return wi, f32(1), tuple(f32(f32(F * r) / ac) for r in self.R)


class SpecularTransmission:
    type = BSDF_TRANSMISSION | BSDF_SPECULAR
    key = "chosen_spec_t"

    def __init__(self, T, eta_a, eta_b):
        self.T, self.eta_a, self.eta_b = T, f32(eta_a), f32(eta_b)

    def f(self, wo, wi, mode):
        return ZERO3

    def pdf(self, wo, wi):
        return f32(0)

    def sample(self, wo, u0, u1, mode, stats=None, normals=None):
        entering = wo[2] > 0
        eta_i, eta_t = (self.eta_a, self.eta_b) if entering else (self.eta_b, self.eta_a)
        n = (f32(-0.0), f32(-0.0), f32(-1)) if wo[2] < 0 else (f32(0), f32(0), f32(1))  # Faceforward(Normal3f(0,0,1), wo)
        wi = refract(wo, n, f32(eta_i / eta_t))
        if wi is None:
            _count(stats, "tir_spec_t")
            return ZERO3, f32(0), ZERO3
        F, _ = fr_dielectric(wi[2], self.eta_a, self.eta_b)
        ac = _abs(wi[2])
        out = []
        for t in self.T:
            ft = f32(t * f32(f32(1) - F))
            if mode == RADIANCE:
                ft = f32(ft * f32(f32(eta_i * eta_i) / f32(eta_t * eta_t)))
            with np.errstate(all="ignore"):
                out.append(f32(ft / ac))
        return wi, f32(1), tuple(out)


class LambertianReflection:
    type = BSDF_REFLECTION | BSDF_DIFFUSE
    key = "chosen_lambert_r"

    def __init__(self, R):
        self.R = R

    def f(self, wo, wi, mode):
        return tuple(f32(r * INV_PI) for r in self.R)

    def pdf(self, wo, wi):
        return f32(_abs(wi[2]) * INV_PI) if _same_hemisphere(wo, wi) else f32(0)

    def sample(self, wo, u0, u1, mode, stats=None, normals=None):
        wi = list(cosine_hemisphere(u0, u1))
        if wo[2] < 0:
            wi[2] = f32(wi[2] * f32(-1))
        wi = tuple(wi)
        return wi, self.pdf(wo, wi), self.f(wo, wi, mode)


class LambertianTransmission(LambertianReflection):
    type = BSDF_TRANSMISSION | BSDF_DIFFUSE
    key = "chosen_lambert_t"

    def pdf(self, wo, wi):
        return f32(_abs(wi[2]) * INV_PI) if not _same_hemisphere(wo, wi) else f32(0)

    def sample(self, wo, u0, u1, mode, stats=None, normals=None):
        wi = list(cosine_hemisphere(u0, u1))
        if wo[2] > 0:
            wi[2] = f32(wi[2] * f32(-1))
        wi = tuple(wi)
        return wi, self.pdf(wo, wi), self.f(wo, wi, mode)


class MicrofacetReflection:
    """Under FresnelDielectric(eta_a, eta_b)."""
    type = BSDF_REFLECTION | BSDF_GLOSSY
    key = "chosen_micro_r"

    def __init__(self, R, ax, ay, eta_a, eta_b):
        self.R, self.ax, self.ay, self.eta_a, self.eta_b = R, f32(ax), f32(ay), f32(eta_a), f32(eta_b)

    def f(self, wo, wi, mode):
        cos_o, cos_i = _abs(wo[2]), _abs(wi[2])
        wh = add(wi, wo)
        if cos_i == 0 or cos_o == 0:
            return ZERO3
        if wh[0] == 0 and wh[1] == 0 and wh[2] == 0:
            return ZERO3
        wh = normalize(wh)
        F, _ = fr_dielectric(dot(wi, wh), self.eta_a, self.eta_b)
        D, G = tr_D(self.ax, self.ay, wh), tr_G(self.ax, self.ay, wo, wi)
        with np.errstate(all="ignore"):
            den = f32(f32(f32(4) * cos_i) * cos_o)
            return tuple(f32(f32(f32(f32(r * D) * G) * F) / den) for r in self.R)

    def pdf(self, wo, wi):
        if not _same_hemisphere(wo, wi):
            return f32(0)
        wh = normalize(add(wo, wi))
        return _divf(tr_pdf(self.ax, self.ay, wo, wh), f32(f32(4) * dot(wo, wh)))

    def sample(self, wo, u0, u1, mode, stats=None, normals=None):
        wh = tr_sample_wh(self.ax, self.ay, wo, u0, u1, stats, normals)
        with np.errstate(all="ignore"):
            wi = _reflect(wo, wh)
        if not _same_hemisphere(wo, wi):
            _count(stats, "micro_r_other_hemisphere")
            return wi, f32(0), ZERO3
        pdf = _divf(tr_pdf(self.ax, self.ay, wo, wh), f32(f32(4) * dot(wo, wh)))
        return wi, pdf, self.f(wo, wi, mode)


class MicrofacetTransmission:
    type = BSDF_TRANSMISSION | BSDF_GLOSSY
    key = "chosen_micro_t"

    def __init__(self, T, ax, ay, eta_a, eta_b):
        self.T, self.ax, self.ay, self.eta_a, self.eta_b = T, f32(ax), f32(ay), f32(eta_a), f32(eta_b)

    def _eta(self, wo):
        return f32(self.eta_b / self.eta_a) if wo[2] > 0 else f32(self.eta_a / self.eta_b)

    def f(self, wo, wi, mode, stats=None):
        if _same_hemisphere(wo, wi):
            return ZERO3
        cos_o, cos_i = wo[2], wi[2]
        if cos_i == 0 or cos_o == 0:
            return ZERO3
        eta = self._eta(wo)
        with np.errstate(all="ignore"):
            wh = normalize(add(wo, mul(wi, eta)))
            if wh[2] < 0:
                _count(stats, "wh_flipped")
                wh = _neg(wh)
            F, _ = fr_dielectric(dot(wo, wh), self.eta_a, self.eta_b)
            sd = f32(dot(wo, wh) + f32(eta * dot(wi, wh)))
            factor = f32(f32(1) / eta) if mode == RADIANCE else f32(1)
            num = f32(tr_D(self.ax, self.ay, wh) * tr_G(self.ax, self.ay, wo, wi))
            for x in (eta, eta, _abs(dot(wi, wh)), _abs(dot(wo, wh)), factor, factor):
                num = f32(num * x)
            den = f32(f32(f32(cos_i * cos_o) * sd) * sd)
            v = _abs(f32(num / den))
            return tuple(f32(f32(f32(f32(1) - F) * t) * v) for t in self.T)

    def pdf(self, wo, wi):
        if _same_hemisphere(wo, wi):
            return f32(0)
        eta = self._eta(wo)
        with np.errstate(all="ignore"):
            wh = normalize(add(wo, mul(wi, eta)))
            sd = f32(dot(wo, wh) + f32(eta * dot(wi, wh)))
            dwh_dwi = _abs(f32(f32(f32(eta * eta) * dot(wi, wh)) / f32(sd * sd)))
            return f32(tr_pdf(self.ax, self.ay, wo, wh) * dwh_dwi)

    def sample(self, wo, u0, u1, mode, stats=None, normals=None):
        wh = tr_sample_wh(self.ax, self.ay, wo, u0, u1, stats, normals)
        eta = f32(self.eta_a / self.eta_b) if wo[2] > 0 else f32(self.eta_b / self.eta_a)
        with np.errstate(all="ignore"):
            wi = refract(wo, wh, eta)
        if wi is None:
            _count(stats, "tir_micro_t")
            return ZERO3, f32(0), ZERO3
        return wi, self.pdf(wo, wi), self.f(wo, wi, mode, stats)


class FresnelBlend:
    type = BSDF_REFLECTION | BSDF_GLOSSY
    key = "chosen_blend"

    def __init__(self, Rd, Rs, ax, ay):
        self.Rd, self.Rs, self.ax, self.ay = Rd, Rs, f32(ax), f32(ay)

    def f(self, wo, wi, mode):
        a = f32(f32(1) - _pow5(f32(f32(1) - f32(f32(0.5) * _abs(wi[2])))))
        b = f32(f32(1) - _pow5(f32(f32(1) - f32(f32(0.5) * _abs(wo[2])))))
        k = f32(f32(28) / f32(f32(23) * PI))
        diffuse = tuple(f32(f32(f32(f32(k * rd) * f32(f32(1) - rs)) * a) * b) for rd, rs in zip(self.Rd, self.Rs))
        wh = add(wi, wo)
        if wh[0] == 0 and wh[1] == 0 and wh[2] == 0:
            return ZERO3
        wh = normalize(wh)
        with np.errstate(all="ignore"):
            sc = f32(tr_D(self.ax, self.ay, wh) /
                     f32(f32(f32(4) * _abs(dot(wi, wh))) * _max(_abs(wi[2]), _abs(wo[2]))))
            p5 = _pow5(f32(f32(1) - dot(wi, wh)))
            spec = tuple(f32(sc * f32(rs + f32(p5 * f32(f32(1) - rs)))) for rs in self.Rs)
            return tuple(f32(d + s) for d, s in zip(diffuse, spec))

    def pdf(self, wo, wi):
        if not _same_hemisphere(wo, wi):
            return f32(0)
        wh = normalize(add(wo, wi))
        pdf_wh = tr_pdf(self.ax, self.ay, wo, wh)
        with np.errstate(all="ignore"):
            return f32(f32(0.5) * f32(f32(_abs(wi[2]) * INV_PI) + f32(pdf_wh / f32(f32(4) * dot(wo, wh)))))

    def sample(self, wo, u0, u1, mode, stats=None, normals=None):
        if u0 < f32(0.5):
            _count(stats, "blend_diffuse_half")
            v = f32(f32(2) * u0)
            v = v if v < ONE_MINUS_EPS else ONE_MINUS_EPS
            wi = list(cosine_hemisphere(v, u1))
            if wo[2] < 0:
                wi[2] = f32(wi[2] * f32(-1))
            wi = tuple(wi)
        else:
            _count(stats, "blend_specular_half")
            v = f32(f32(2) * f32(u0 - f32(0.5)))
            v = v if v < ONE_MINUS_EPS else ONE_MINUS_EPS
            wh = tr_sample_wh(self.ax, self.ay, wo, v, u1, stats, normals)
            with np.errstate(all="ignore"):
                wi = _reflect(wo, wh)
            if not _same_hemisphere(wo, wi):
                _count(stats, "blend_other_hemisphere")
                return wi, f32(0), ZERO3
        return wi, self.pdf(wo, wi), self.f(wo, wi, mode)


def _black(c):
    return all(x == 0 for x in c)


def _mul3(a, b):
    return tuple(f32(x * y) for x, y in zip(a, b))


def _alpha(r, remap):
    return rb.roughness_to_alpha(f32(r)) if remap else f32(r)


# ---- the BSDF of a material ----
class FullBsdf:
    """A bre_material_ex of type rough glass / uber / translucent / substrate as its ComputeScatteringFunctions
    leaves the BSDF: self.lobes, the BxDFs in the order added."""

    def __init__(self, kind, kd=ZERO3, ks=ZERO3, kr=ZERO3, kt=ZERO3, eta=1.5, roughness=0.1, uroughness=0.0,
                 vroughness=0.0, opacity=(1, 1, 1), remap=True):
        self.kind = int(kind)
        kd, ks, kr, kt = (tuple(_clamp01(x) for x in c) for c in (kd, ks, kr, kt))
        eta = f32(eta)
        L = self.lobes = []
        if self.kind == ROUGH_GLASS:  # glass.cpp:54-91
            R, T = kr, kt
            if not (_black(R) and _black(T)):
                u, v = _alpha(uroughness, remap), _alpha(vroughness, remap)
                if not _black(R):
                    L.append(MicrofacetReflection(R, u, v, 1, eta))
                if not _black(T):
                    L.append(MicrofacetTransmission(T, u, v, 1, eta))
        elif self.kind == UBER:  # uber.cpp:51-100
            op = tuple(_clamp01(x) for x in opacity)
            t = tuple(_max(f32(f32(-x) + f32(1)), f32(0)) for x in op)  # (-op + Spectrum(1.f)).Clamp()
            if not _black(t):
                L.append(SpecularTransmission(t, 1, 1))
            c = _mul3(op, kd)
            if not _black(c):
                L.append(LambertianReflection(c))
            c = _mul3(op, ks)
            if not _black(c):
                ru = f32(uroughness) if f32(uroughness) != 0 else f32(roughness)
                rv = f32(vroughness) if f32(vroughness) != 0 else ru
                L.append(MicrofacetReflection(c, _alpha(ru, remap), _alpha(rv, remap), 1, eta))
            c = _mul3(op, kr)
            if not _black(c):
                L.append(SpecularReflection(c, 1, eta))
            c = _mul3(op, kt)
            if not _black(c):
                L.append(SpecularTransmission(c, 1, eta))
        elif self.kind == TRANSLUCENT:  # translucent.cpp:50-79
            r, t = kr, kt
            if not (_black(r) and _black(t)):
                if not _black(kd):
                    if not _black(r):
                        L.append(LambertianReflection(_mul3(r, kd)))
                    if not _black(t):
                        L.append(LambertianTransmission(_mul3(t, kd)))
                if not _black(ks):
                    a = _alpha(roughness, remap)
                    if not _black(r):
                        L.append(MicrofacetReflection(_mul3(r, ks), a, a, 1, 1.5))
                    if not _black(t):
                        L.append(MicrofacetTransmission(_mul3(t, ks), a, a, 1, 1.5))
        else:  # substrate.cpp:51-64
            assert self.kind == SUBSTRATE
            if not _black(kd) or not _black(ks):
                L.append(FresnelBlend(kd, ks, _alpha(uroughness, remap), _alpha(vroughness, remap)))
        self.none = not L

    @classmethod
    def of(cls, m):
        """From a scene.MaterialEx."""
        return cls(m.type, m.kd, m.ks, m.kr, m.kt, m.eta, m.roughness, m.uroughness, m.vroughness, m.opacity,
                   bool(m.remap))

    def matching(self, flags):
        return [b for b in self.lobes if (b.type & flags) == b.type]  # BxDF::MatchesFlags

    def _sum_f(self, lobes, reflect, wo, wi, mode):
        f = ZERO3
        side = BSDF_REFLECTION if reflect else BSDF_TRANSMISSION
        for b in lobes:
            if b.type & side:
                with np.errstate(all="ignore"):
                    f = add(f, b.f(wo, wi, mode))
        return f

    # ---- BSDF::f, Pdf, Sample_f on world vectors with the triangle `q` (its ss, ts, n; ng = n) ----
    def f(self, q, wo_w, wi_w, flags=BSDF_ALL, mode=RADIANCE):
        wi, wo = rb._to_local(q, wi_w), rb._to_local(q, wo_w)
        if wo[2] == 0:
            return ZERO3
        reflect = f32(dot(wi_w, q["n"]) * dot(wo_w, q["n"])) > 0
        return self._sum_f(self.matching(flags), reflect, wo, wi, mode)

    def pdf(self, q, wo_w, wi_w, flags=BSDF_ALL):
        if not self.lobes:
            return f32(0)
        wo, wi = rb._to_local(q, wo_w), rb._to_local(q, wi_w)
        if wo[2] == 0:
            return f32(0)
        pdf = f32(0)
        match = self.matching(flags)
        for b in match:
            with np.errstate(all="ignore"):
                pdf = f32(pdf + b.pdf(wo, wi))
        return _divf(pdf, f32(len(match))) if match else f32(0)

    def sample(self, q, wo_w, u0, u1, flags=BSDF_ALL, mode=RADIANCE, stats=None, normals=None):
        """BSDF::Sample_f(wo, ., (u0, u1), ., flags, .): (wi world, pdf, f, sampled type), or None where it returns 0
        before f is known (no matching BxDF, wo.z == 0, pdf == 0)."""
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
        wi, pdf, f = b.sample(wo, ur, u1, mode, stats, normals)
        if pdf == 0:
            return None
        wi_w = to_world(q, wi)
        specular = bool(b.type & BSDF_SPECULAR)
        if len({bool(x.type & BSDF_SPECULAR) for x in match}) == 2:
            _count(stats, "sampled_specular_of_mixed" if specular else "sampled_nonspecular_of_mixed")
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
        return wi_w, pdf, f, b.type


def bsdf_of(m):
    """The restated BSDF of a scene.MaterialEx of type >= 4: refpy_bsdf.Bsdf or FullBsdf, behind one calling
    convention f(q, wo, wi, flags, mode), pdf(q, wo, wi, flags), sample(q, wo, u0, u1, flags, mode, stats, normals).
    A plastic, metal or matte has no specular and no transmitting lobe: flags and mode change nothing for it."""
    if m.type >= ROUGH_GLASS:
        return FullBsdf.of(m)
    return _Glossy(rb.Bsdf.of(m))


class _Glossy:
    def __init__(self, b):
        self.b, self.none, self.lobes = b, b.none, b.lobes

    def matching(self, flags):
        return self.lobes

    def f(self, q, wo, wi, flags=BSDF_ALL, mode=RADIANCE):
        return self.b.f(q, wo, wi)

    def pdf(self, q, wo, wi, flags=BSDF_ALL):
        return self.b.pdf(q, wo, wi)

    def sample(self, q, wo, u0, u1, flags=BSDF_ALL, mode=RADIANCE, stats=None, normals=None):
        return self.b.sample(q, wo, u0, u1, stats, normals)
