"""Plastic, metal and rough matte of the pure-Python float32 restatement (test infrastructure), each from the
reference text:
* the materials: PlasticMaterial::ComputeScatteringFunctions (src/materials/plastic.cpp:45-70), MetalMaterial's
  (src/materials/metal.cpp:59-80), MatteMaterial's (src/materials/matte.cpp:45-62), with
  TrowbridgeReitzDistribution::RoughnessToAlpha (src/core/microfacet.h:123-128) and OrenNayar's constructor
  (src/core/reflection.h:417-423);
* the lobes: LambertianReflection::f (src/core/reflection.cpp:178-180), OrenNayar::f (:197-219), both sampled by
  BxDF::Sample_f / Pdf (:378-389); MicrofacetReflection::f / Sample_f / Pdf (:226-236, 405-423) over
  TrowbridgeReitzDistribution D, Lambda, Sample_wh and MicrofacetDistribution::G1, G, Pdf
  (src/core/microfacet.cpp:155-163, 176-184, 238-344; microfacet.h:54-60), FrDielectric (refpy_specular) and
  FrConductor (reflection.cpp:71-95, 118-120);
* the BSDF: BSDF::f (:670-683), BSDF::Pdf (:770-785), BSDF::Sample_f (:703-768).
Every float operation is done on numpy float32 scalars in the reference's order, with one exception, which is the
reference's own: TrowbridgeReitzSample11's normal-incidence branch (microfacet.cpp:241-247) compares against a
double and calls sqrt, cos and sin unqualified on Floats, which under libstdc++ are the double functions: math.sqrt,
math.cos and math.sin here, the host libm.

`stats`, a dict from new_stats(), counts the branches taken (COUNTERS); `normals`, a list, receives (r, phi) of
every normal-incidence sample, for the midpoint-margin check.
"""
from __future__ import annotations

import math

import numpy as np

from refpy_photon import INV_PI, ONE_MINUS_EPS, PI, add, cosine_hemisphere, div, dot, f32, length, logf, mul, normalize
from refpy_specular import ZERO3, fr_dielectric, to_world

MATTE, PLASTIC, METAL = 4, 5, 6
BSDF_REFLECTION, BSDF_DIFFUSE, BSDF_GLOSSY = 1, 4, 8
LAMBERT, OREN, MICRO = "lambert", "oren", "micro"

COUNTERS = ("lobe_first", "lobe_second", "sample11_normal", "sample11_general", "slope_x_1", "slope_x_2", "u2_upper",
            "u2_lower", "wi_other_hemisphere", "oren_maxcos", "oren_alpha_o", "oren_alpha_i", "fr_tir_15")


def new_stats():
    return {k: 0 for k in COUNTERS}


def _count(stats, key):
    if stats is not None:
        stats[key] += 1


def _clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)  # pbrt.h:278-284


def _clamp01(v):
    return _clamp(f32(v), f32(0), f32(1))


def _max(a, b):
    return b if a < b else a  # std::max(a, b)


def _sqrt(x):
    with np.errstate(invalid="ignore"):
        return f32(np.sqrt(f32(x)))


def _divf(a, b):
    with np.errstate(all="ignore"):
        return f32(f32(a) / f32(b))


# ---- reflection.h:56-83 ----
def cos2_theta(w):
    return f32(w[2] * w[2])


def sin2_theta(w):
    return _max(f32(0), f32(f32(1) - cos2_theta(w)))


def sin_theta(w):
    return _sqrt(sin2_theta(w))


def tan_theta(w):
    return _divf(sin_theta(w), w[2])


def tan2_theta(w):
    return _divf(sin2_theta(w), cos2_theta(w))


def cos_phi(w):
    s = sin_theta(w)
    return f32(1) if s == 0 else _clamp(_divf(w[0], s), f32(-1), f32(1))


def sin_phi(w):
    s = sin_theta(w)
    return f32(0) if s == 0 else _clamp(_divf(w[1], s), f32(-1), f32(1))


# ---- the Trowbridge-Reitz distribution ----
def roughness_to_alpha(roughness):
    roughness = _max(f32(roughness), f32(1e-3))
    x = logf(roughness)
    v = f32(f32(1.62142) + f32(f32(0.819955) * x))
    v = f32(v + f32(f32(f32(0.1734) * x) * x))
    v = f32(v + f32(f32(f32(f32(0.0171201) * x) * x) * x))
    return f32(v + f32(f32(f32(f32(f32(0.000640711) * x) * x) * x) * x))


def tr_D(ax, ay, wh):
    tan2 = tan2_theta(wh)
    if np.isinf(tan2):
        return f32(0)
    cos4 = f32(cos2_theta(wh) * cos2_theta(wh))
    cp, sp = cos_phi(wh), sin_phi(wh)
    e = f32(f32(_divf(f32(cp * cp), f32(ax * ax)) + _divf(f32(sp * sp), f32(ay * ay))) * tan2)
    with np.errstate(all="ignore"):
        one_e = f32(f32(1) + e)
        den = f32(f32(f32(f32(f32(PI * ax) * ay) * cos4) * one_e) * one_e)
    return _divf(f32(1), den)


def tr_lambda(ax, ay, w):
    abs_tan = f32(abs(tan_theta(w)))
    if np.isinf(abs_tan):
        return f32(0)
    cp, sp = cos_phi(w), sin_phi(w)
    alpha = _sqrt(f32(f32(f32(f32(cp * cp) * ax) * ax) + f32(f32(f32(sp * sp) * ay) * ay)))
    with np.errstate(all="ignore"):
        at = f32(alpha * abs_tan)
        a2t2 = f32(at * at)
        return f32(f32(f32(-1) + _sqrt(f32(f32(1) + a2t2))) / f32(2))


def tr_G1(ax, ay, w):
    return _divf(f32(1), f32(f32(1) + tr_lambda(ax, ay, w)))


def tr_G(ax, ay, wo, wi):
    return _divf(f32(1), f32(f32(f32(1) + tr_lambda(ax, ay, wo)) + tr_lambda(ax, ay, wi)))


def tr_sample11(cos_t, U1, U2, stats=None, normals=None):
    """TrowbridgeReitzSample11, microfacet.cpp:238-282 (without its CHECKs): (slope_x, slope_y)."""
    if float(cos_t) > .9999:
        _count(stats, "sample11_normal")
        r = f32(math.sqrt(float(_divf(U1, f32(f32(1) - U1)))))
        phi = f32(6.28318530718 * float(U2))
        if normals is not None:
            normals.append((r, phi))
        return f32(float(r) * math.cos(float(phi))), f32(float(r) * math.sin(float(phi)))
    _count(stats, "sample11_general")
    sin_t = _sqrt(_max(f32(0), f32(f32(1) - f32(cos_t * cos_t))))
    tan_t = _divf(sin_t, cos_t)
    a = _divf(f32(1), tan_t)
    with np.errstate(all="ignore"):
        G1 = f32(f32(2) / f32(f32(1) + _sqrt(f32(f32(1) + f32(f32(1) / f32(a * a))))))
        A = f32(f32(f32(f32(2) * U1) / G1) - f32(1))
        tmp = f32(f32(1) / f32(f32(A * A) - f32(1)))
        if float(tmp) > 1e10:
            tmp = f32(1e10)
        B = tan_t
        inner = f32(f32(f32(f32(B * B) * tmp) * tmp) - f32(f32(f32(A * A) - f32(B * B)) * tmp))
        D = _sqrt(_max(inner, f32(0)))
        sx1 = f32(f32(B * tmp) - D)
        sx2 = f32(f32(B * tmp) + D)
        first = A < 0 or sx2 > f32(f32(1) / tan_t)
        _count(stats, "slope_x_1" if first else "slope_x_2")
        slope_x = sx1 if first else sx2
        if U2 > f32(0.5):
            _count(stats, "u2_upper")
            S = f32(1)
            U2 = f32(f32(2) * f32(U2 - f32(0.5)))
        else:
            _count(stats, "u2_lower")
            S = f32(-1)
            U2 = f32(f32(2) * f32(f32(0.5) - U2))
        num = f32(U2 * f32(f32(U2 * f32(f32(U2 * f32(0.27385)) - f32(0.73369))) + f32(0.46341)))
        den = f32(f32(U2 * f32(f32(U2 * f32(f32(U2 * f32(0.093073)) + f32(0.309420))) - f32(1.000000))) + f32(0.597999))
        z = f32(num / den)
        slope_y = f32(f32(S * z) * _sqrt(f32(f32(1) + f32(slope_x * slope_x))))
    return slope_x, slope_y


def tr_sample_wh(ax, ay, wo, u0, u1, stats=None, normals=None):
    """TrowbridgeReitzDistribution::Sample_wh, sampleVisibleArea (microfacet.cpp:330-334) over
    TrowbridgeReitzSample (:284-305)."""
    flip = wo[2] < 0
    wi = tuple(-x for x in wo) if flip else wo
    ws = normalize((f32(ax * wi[0]), f32(ay * wi[1]), wi[2]))
    sx, sy = tr_sample11(ws[2], u0, u1, stats, normals)
    cp, sp = cos_phi(ws), sin_phi(ws)
    with np.errstate(all="ignore"):
        tmp = f32(f32(cp * sx) - f32(sp * sy))
        sy = f32(f32(sp * sx) + f32(cp * sy))
        sx = tmp
        sx = f32(ax * sx)
        sy = f32(ay * sy)
        wh = normalize((-sx, -sy, f32(1)))
    return tuple(-x for x in wh) if flip else wh


def tr_pdf(ax, ay, wo, wh):
    with np.errstate(all="ignore"):
        return f32(f32(f32(tr_D(ax, ay, wh) * tr_G1(ax, ay, wo)) * f32(abs(dot(wo, wh)))) / f32(abs(wo[2])))


def fr_conductor(cos_i, etat, k):
    """FrConductor, reflection.cpp:71-95, one channel, etai = 1."""
    cos_i = _clamp(cos_i, f32(-1), f32(1))
    eta, etak = f32(etat / f32(1)), f32(k / f32(1))
    cos2 = f32(cos_i * cos_i)
    sin2 = f32(1. - float(cos2))
    eta2, etak2 = f32(eta * eta), f32(etak * etak)
    with np.errstate(all="ignore"):
        t0 = f32(f32(eta2 - etak2) - sin2)
        a2b2 = _sqrt(f32(f32(t0 * t0) + f32(f32(eta2 * f32(4)) * etak2)))
        t1 = f32(a2b2 + cos2)
        a = _sqrt(f32(f32(a2b2 + t0) * f32(0.5)))
        t2 = f32(a * f32(f32(2) * cos_i))
        Rs = f32(f32(t1 - t2) / f32(t1 + t2))
        t3 = f32(f32(a2b2 * cos2) + f32(sin2 * sin2))
        t4 = f32(t2 * sin2)
        Rp = f32(f32(Rs * f32(t3 - t4)) / f32(t3 + t4))
        return f32(f32(Rp + Rs) * f32(0.5))


# ---- the BSDF of a material ----
class Bsdf:
    """A bre_material_ex of type matte / plastic / metal as its ComputeScatteringFunctions leaves the BSDF:
    self.lobes, the BxDFs in the order added (LAMBERT, OREN, MICRO)."""

    def __init__(self, kind, kd=ZERO3, ks=ZERO3, ceta=ZERO3, ck=ZERO3, roughness=0.1, uroughness=0.0, vroughness=0.0,
                 sigma=0.0, remap=True):
        self.kind = int(kind)
        self.kd = tuple(_clamp01(x) for x in kd)
        self.ks = tuple(_clamp01(x) for x in ks)
        self.ceta = tuple(f32(x) for x in ceta)
        self.ck = tuple(f32(x) for x in ck)
        self.lobes = []
        self.ax = self.ay = f32(1)
        self.A = self.B = f32(0)
        self.conductor = False
        if self.kind == MATTE:
            sig = _clamp(f32(sigma), f32(0), f32(90))
            if any(x != 0 for x in self.kd):
                self.lobes.append(LAMBERT if sig == 0 else OREN)
            if sig != 0:
                s = f32(f32(PI / f32(180)) * sig)  # Radians, pbrt.h:295
                s2 = f32(s * s)
                self.A = f32(f32(1) - f32(s2 / f32(f32(2) * f32(s2 + f32(0.33)))))
                self.B = f32(f32(f32(0.45) * s2) / f32(s2 + f32(0.09)))
        elif self.kind == PLASTIC:
            if any(x != 0 for x in self.kd):
                self.lobes.append(LAMBERT)
            if any(x != 0 for x in self.ks):
                self.lobes.append(MICRO)
            rough = f32(roughness)
            if remap:
                rough = roughness_to_alpha(rough)
            self.ax = self.ay = rough
            self.conductor = False
        else:
            assert self.kind == METAL
            u = f32(uroughness) if f32(uroughness) != 0 else f32(roughness)
            v = f32(vroughness) if f32(vroughness) != 0 else f32(roughness)
            if remap:
                u, v = roughness_to_alpha(u), roughness_to_alpha(v)
            self.ax, self.ay = u, v
            self.ks = (f32(1),) * 3
            self.lobes.append(MICRO)
            self.conductor = True
        self.none = not self.lobes

    @classmethod
    def of(cls, m):
        """From a scene.MaterialEx."""
        return cls(m.type, m.kd, m.ks, m.ceta, m.ck, m.roughness, m.uroughness, m.vroughness, m.sigma, bool(m.remap))

    # ---- the lobes, in the shading frame ----
    def lobe_type(self, lobe):
        return BSDF_REFLECTION | (BSDF_GLOSSY if lobe == MICRO else BSDF_DIFFUSE)

    def lobe_f(self, lobe, wo, wi, stats=None):
        if lobe == LAMBERT:
            return tuple(f32(k * INV_PI) for k in self.kd)
        if lobe == OREN:
            sin_i, sin_o = sin_theta(wi), sin_theta(wo)
            max_cos = f32(0)
            if float(sin_i) > 1e-4 and float(sin_o) > 1e-4:
                d_cos = f32(f32(cos_phi(wi) * cos_phi(wo)) + f32(sin_phi(wi) * sin_phi(wo)))
                max_cos = _max(f32(0), d_cos)
                if max_cos > 0:
                    _count(stats, "oren_maxcos")
            if abs(wi[2]) > abs(wo[2]):
                _count(stats, "oren_alpha_o")
                sin_alpha = sin_o
                tan_beta = _divf(sin_i, f32(abs(wi[2])))
            else:
                _count(stats, "oren_alpha_i")
                sin_alpha = sin_i
                tan_beta = _divf(sin_o, f32(abs(wo[2])))
            with np.errstate(all="ignore"):
                s = f32(self.A + f32(f32(f32(self.B * max_cos) * sin_alpha) * tan_beta))
                return tuple(f32(f32(k * INV_PI) * s) for k in self.kd)
        cos_o, cos_i = f32(abs(wo[2])), f32(abs(wi[2]))
        wh = add(wi, wo)
        if cos_i == 0 or cos_o == 0:
            return ZERO3
        if wh[0] == 0 and wh[1] == 0 and wh[2] == 0:
            return ZERO3
        wh = normalize(wh)
        ci = dot(wi, wh)
        if self.conductor:
            F = tuple(fr_conductor(f32(abs(ci)), self.ceta[c], self.ck[c]) for c in range(3))
        else:
            Fd, tir = fr_dielectric(ci, f32(1.5), f32(1))
            if tir:
                _count(stats, "fr_tir_15")
            F = (Fd,) * 3
        D, G = tr_D(self.ax, self.ay, wh), tr_G(self.ax, self.ay, wo, wi)
        with np.errstate(all="ignore"):
            den = f32(f32(f32(4) * cos_i) * cos_o)
            return tuple(f32(f32(f32(f32(self.ks[c] * D) * G) * F[c]) / den) for c in range(3))

    def lobe_pdf(self, lobe, wo, wi):
        if lobe != MICRO:
            return f32(abs(wi[2]) * INV_PI) if f32(wo[2] * wi[2]) > 0 else f32(0)
        if not f32(wo[2] * wi[2]) > 0:
            return f32(0)
        wh = normalize(add(wo, wi))
        return _divf(tr_pdf(self.ax, self.ay, wo, wh), f32(f32(4) * dot(wo, wh)))

    def lobe_sample(self, lobe, wo, u0, u1, stats=None, normals=None):
        """(wi, pdf, f); pdf = 0 where the lobe returns early (it arrived as 0)."""
        if lobe != MICRO:
            wi = list(cosine_hemisphere(u0, u1))
            if wo[2] < 0:
                wi[2] = f32(wi[2] * f32(-1))
            wi = tuple(wi)
            return wi, self.lobe_pdf(lobe, wo, wi), self.lobe_f(lobe, wo, wi, stats)
        wh = tr_sample_wh(self.ax, self.ay, wo, u0, u1, stats, normals)
        with np.errstate(all="ignore"):
            wi = add(tuple(-x for x in wo), mul(wh, f32(f32(2) * dot(wo, wh))))  # Reflect, reflection.h:92-94
        if not f32(wo[2] * wi[2]) > 0:
            _count(stats, "wi_other_hemisphere")
            return wi, f32(0), ZERO3
        pdf = _divf(tr_pdf(self.ax, self.ay, wo, wh), f32(f32(4) * dot(wo, wh)))
        return wi, pdf, self.lobe_f(lobe, wo, wi, stats)

    # ---- BSDF::f, Pdf, Sample_f on world vectors with the triangle `q` (its ss, ts, n; ng = n) ----
    def f(self, q, wo_w, wi_w, stats=None):
        wi, wo = _to_local(q, wi_w), _to_local(q, wo_w)
        if wo[2] == 0:
            return ZERO3
        reflect = f32(dot(wi_w, q["n"]) * dot(wo_w, q["n"])) > 0
        f = ZERO3
        for lobe in self.lobes:
            if reflect:  # every lobe is a BSDF_REFLECTION
                with np.errstate(all="ignore"):
                    f = add(f, self.lobe_f(lobe, wo, wi, stats))
        return f

    def pdf(self, q, wo_w, wi_w):
        if not self.lobes:
            return f32(0)
        wo, wi = _to_local(q, wo_w), _to_local(q, wi_w)
        if wo[2] == 0:
            return f32(0)
        pdf = f32(0)
        for lobe in self.lobes:
            with np.errstate(all="ignore"):
                pdf = f32(pdf + self.lobe_pdf(lobe, wo, wi))
        return _divf(pdf, f32(len(self.lobes)))

    def sample(self, q, wo_w, u0, u1, stats=None, normals=None):
        """BSDF::Sample_f(wo, ., (u0, u1), ., BSDF_ALL, .): (wi world, pdf, f, type), or None where it returns 0
        before f is known (no BxDF, wo.z == 0, pdf == 0)."""
        n = len(self.lobes)
        if n == 0:
            return None
        u0, u1 = f32(u0), f32(u1)
        comp = min(int(math.floor(f32(u0 * f32(n)))), n - 1)
        lobe = self.lobes[comp]
        ur = f32(f32(u0 * f32(n)) - f32(comp))
        ur = ur if ur < ONE_MINUS_EPS else ONE_MINUS_EPS  # std::min(., OneMinusEpsilon)
        wo = _to_local(q, wo_w)
        if wo[2] == 0:
            return None
        if n > 1:
            _count(stats, "lobe_first" if comp == 0 else "lobe_second")
        wi, pdf, f = self.lobe_sample(lobe, wo, ur, u1, stats, normals)
        if pdf == 0:
            return None
        wi_w = to_world(q, wi)
        if n > 1:
            with np.errstate(all="ignore"):
                for other in self.lobes:
                    if other != lobe:
                        pdf = f32(pdf + self.lobe_pdf(other, wo, wi))
                pdf = f32(pdf / f32(n))
                reflect = f32(dot(wi_w, q["n"]) * dot(wo_w, q["n"])) > 0
                f = ZERO3
                for l2 in self.lobes:
                    if reflect:
                        f = add(f, self.lobe_f(l2, wo, wi, stats))
        return wi_w, pdf, f, self.lobe_type(lobe)


def _to_local(q, v):
    return (dot(v, q["ss"]), dot(v, q["ts"]), dot(v, q["n"]))


FRAME = dict(ss=(f32(1), f32(0), f32(0)), ts=(f32(0), f32(1), f32(0)), n=(f32(0), f32(0), f32(1)))


# ---- the midpoint margin of the normal-incidence branch ----
def midpoint_margin(x):
    """The relative distance of the double x from the nearest float32 rounding midpoint (inf for 0 and for values
    that round in the subnormal range, where the spacing is absolute)."""
    x = abs(float(x))
    if x == 0 or x < 2.0 ** -126:
        return math.inf
    m, e = math.frexp(x)          # x = m 2^e, m in [0.5, 1)
    t = m * 2.0 ** 24             # in [2^23, 2^24): float32 values are the integers, midpoints the half-integers
    frac = t - math.floor(t)
    return abs(frac - 0.5) / t
