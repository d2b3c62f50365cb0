"""Mirror and glass of the pure-Python float32 restatement (test infrastructure), each from the reference text:
* FrDielectric (src/core/reflection.cpp:47-68), Refract (reflection.h:96-108);
* SpecularReflection::Sample_f (reflection.cpp:136-143) and FresnelSpecular::Sample_f (:477-511) inside
  BSDF::Sample_f (:703-768) for a BSDF with that one lobe (MirrorMaterial, mirror.cpp:45-56; GlassMaterial
  with zero roughness and allowMultipleLobes, glass.cpp:45-65): TransportMode::Importance for photons,
  Radiance for the camera.
Every float operation is done on numpy float32 scalars in the reference's order.
"""
from __future__ import annotations

import numpy as np

from refpy_photon import f32

MIRROR, GLASS, INTERFACE = 1, 2, 3
BSDF_REFLECTION, BSDF_TRANSMISSION, BSDF_SPECULAR = 1, 2, 16
IMPORTANCE, RADIANCE = 0, 1
ZERO3 = (f32(0),) * 3


def _max0(x):
    return x if f32(0) < x else f32(0)  # std::max((Float)0, x)


def _clamp01(v):
    v = f32(v)
    return f32(0) if v < 0 else (f32(1) if v > 1 else v)


class Mat:
    """A bre_material as bre_set_materials keeps it: Kr and Kt clamped to [0, 1]."""

    def __init__(self, kind, kr, kt, eta):
        self.kind = int(kind)
        self.kr = tuple(_clamp01(x) for x in kr)
        self.kt = tuple(_clamp01(x) for x in kt)
        self.eta = f32(eta)
        # mirror.cpp:53, glass.cpp:59: no BxDF is added
        self.none = all(x == 0 for x in self.kr) and (self.kind == MIRROR or all(x == 0 for x in self.kt))

    @classmethod
    def of(cls, m):
        return cls(m.type, m.kr, m.kt, m.eta)


def fr_dielectric(cos_i, eta_i, eta_t):
    """FrDielectric, reflection.cpp:47-68: (F, whether it left through `sinThetaT >= 1`)."""
    cos_i = f32(-1) if cos_i < -1 else (f32(1) if cos_i > 1 else cos_i)
    if not cos_i > 0:
        eta_i, eta_t = eta_t, eta_i
        cos_i = f32(abs(cos_i))
    sin_i = f32(np.sqrt(_max0(f32(f32(1) - f32(cos_i * cos_i)))))
    sin_t = f32(f32(eta_i / eta_t) * sin_i)
    if sin_t >= 1:
        return f32(1), True
    cos_t = f32(np.sqrt(_max0(f32(f32(1) - f32(sin_t * sin_t)))))
    a, b = f32(eta_t * cos_i), f32(eta_i * cos_t)
    c, d = f32(eta_i * cos_i), f32(eta_t * cos_t)
    with np.errstate(all="ignore"):
        r_parl = f32(f32(a - b) / f32(a + b))
        r_perp = f32(f32(c - d) / f32(c + d))
        return f32(f32(f32(r_parl * r_parl) + f32(r_perp * r_perp)) / f32(2)), False


def refract(wi, n, eta):
    """Refract, reflection.h:96-108: wt or None."""
    cos_i = f32(f32(f32(n[0] * wi[0]) + f32(n[1] * wi[1])) + f32(n[2] * wi[2]))
    sin2_i = _max0(f32(f32(1) - f32(cos_i * cos_i)))
    sin2_t = f32(f32(eta * eta) * sin2_i)
    if sin2_t >= 1:
        return None
    cos_t = f32(np.sqrt(f32(f32(1) - sin2_t)))
    k = f32(f32(eta * cos_i) - cos_t)
    return tuple(f32(f32(eta * -wi[i]) + f32(k * n[i])) for i in range(3))


def specular_sample(m, wo, u0, mode):
    """BSDF::Sample_f(wo, ., (u0, .), ., BSDF_ALL, .) of the one specular lobe of `m`, wo and wi in the
    shading frame: (wi, pdf, f, type, branch).  Where Sample_f returns 0, pdf = 0, type = 0, wi = f = 0 and
    branch says why ("wo_z0", "refract_fail")."""
    wo = tuple(f32(x) for x in wo)
    u0 = f32(u0)
    if wo[2] == 0:
        return ZERO3, f32(0), ZERO3, 0, "wo_z0"
    refl = (-wo[0], -wo[1], wo[2])
    if m.kind == MIRROR:
        ac = f32(abs(refl[2]))
        with np.errstate(all="ignore"):
            f = tuple(f32(f32(f32(1) * k) / ac) for k in m.kr)
        return refl, f32(1), f, BSDF_SPECULAR | BSDF_REFLECTION, "mirror_reflect"
    F, tir = fr_dielectric(wo[2], f32(1), m.eta)
    if u0 < F:
        ac = f32(abs(refl[2]))
        with np.errstate(all="ignore"):
            f = tuple(f32(f32(k * F) / ac) for k in m.kr)
        return refl, F, f, BSDF_SPECULAR | BSDF_REFLECTION, "tir" if tir else "glass_reflect"
    entering = wo[2] > 0
    eta_i, eta_t = (f32(1), m.eta) if entering else (m.eta, f32(1))
    n = (f32(-0.0), f32(-0.0), f32(-1)) if wo[2] < 0 else (f32(0), f32(0), f32(1))  # Faceforward(Normal3f(0, 0, 1), wo)
    wi = refract(wo, n, f32(eta_i / eta_t))
    if wi is None:
        return ZERO3, f32(0), ZERO3, 0, "refract_fail"
    pdf = f32(f32(1) - F)
    if pdf == 0:
        return ZERO3, f32(0), ZERO3, 0, "pdf0"
    ac = f32(abs(wi[2]))
    f = []
    for k in m.kt:
        ft = f32(k * f32(f32(1) - F))
        if mode == RADIANCE:
            ft = f32(ft * f32(f32(eta_i * eta_i) / f32(eta_t * eta_t)))
        with np.errstate(all="ignore"):
            f.append(f32(ft / ac))
    return wi, pdf, tuple(f), BSDF_SPECULAR | BSDF_TRANSMISSION, "transmit_enter" if entering else "transmit_leave"


def to_world(q, wl):
    ss, ts, n = q["ss"], q["ts"], q["n"]
    return tuple(f32(f32(f32(ss[i] * wl[0]) + f32(ts[i] * wl[1])) + f32(n[i] * wl[2])) for i in range(3))
