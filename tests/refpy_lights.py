"""Point and spot lights of the pure-Python float32 restatement (test infrastructure), each from the
reference text:
* the merged scene.lights order of delta lights and emitting triangles (api.cpp: lights are appended
  in declaration order; bre_light.order = triangles declared before the light);
* Power().y() of a PointLight (src/lights/point.cpp:55) and a SpotLight (src/lights/spot.cpp:75-77);
* PointLight::Sample_Le (point.cpp:61-71), SpotLight::Sample_Le and Falloff (spot.cpp:64-73, 83-93),
  UniformSampleSphere / UniformSampleCone / UniformConePdf (src/core/sampling.cpp:98-103, 132-142).
Every float operation is done on numpy float32 scalars in the reference's order.
"""
from __future__ import annotations

import numpy as np

import refpy_photon as rp
from refpy_photon import PI, f32, normalize

INV_4PI = f32(0.07957747154594766788)
LIGHT_POINT, LIGHT_SPOT = 1, 2


def cosf(x):
    return rp.sincosf(x)[1]


def radians(deg):
    return f32(f32(PI / f32(180)) * f32(deg))  # pbrt.h:295


def lum(s):
    return f32(f32(f32(f32(0.212671) * s[0]) + f32(f32(0.715160) * s[1])) + f32(f32(0.072169) * s[2]))


def xform_vec(m, v):
    """Transform::operator()(Vector3f), transform.h:236-242 (m: 4x4 rows of float32)."""
    return tuple(f32(f32(f32(m[i][0] * v[0]) + f32(m[i][1] * v[1])) + f32(m[i][2] * v[2])) for i in range(3))


def xform_point(m, p):
    """Transform::operator()(Point3f), transform.h:223-233, the wp == 1 test included."""
    r = [f32(f32(f32(f32(m[i][0] * p[0]) + f32(m[i][1] * p[1])) + f32(m[i][2] * p[2])) + m[i][3]) for i in range(4)]
    if r[3] == 1:
        return tuple(r[:3])
    inv = f32(f32(1) / r[3])  # Point3::operator/ multiplies by 1/f
    return tuple(f32(inv * v) for v in r[:3])


class DeltaLight:
    """A bre_light as the reference's PointLight / SpotLight constructors see it."""

    def __init__(self, L):
        self.kind = int(L.type)
        self.I = tuple(f32(x) for x in L.I)
        self.l2w = [[f32(L.light_to_world[4 * i + j]) for j in range(4)] for i in range(4)]
        self.w2l = [[f32(L.world_to_light[4 * i + j]) for j in range(4)] for i in range(4)]
        self.order = int(L.order)
        self.p = xform_point(self.l2w, (f32(0), f32(0), f32(0)))
        self.cos_total = cosf(radians(L.cone_total_deg))
        self.cos_start = cosf(radians(L.cone_falloff_start_deg))

    def power_y(self):
        if self.kind == LIGHT_POINT:  # 4 * Pi * I
            k = f32(f32(4) * PI)
            return lum(tuple(f32(c * k) for c in self.I))
        # I * 2 * Pi * (1 - .5f * (cosFalloffStart + cosTotalWidth))
        k = f32(f32(1) - f32(f32(0.5) * f32(self.cos_start + self.cos_total)))
        return lum(tuple(f32(f32(f32(c * f32(2)) * PI) * k) for c in self.I))

    def falloff(self, w):
        """SpotLight::Falloff, spot.cpp:64-73 (1 for a point light)."""
        if self.kind == LIGHT_POINT:
            return f32(1)
        wl = normalize(xform_vec(self.w2l, w))
        c = wl[2]
        if c < self.cos_total:
            return f32(0)
        if c > self.cos_start:
            return f32(1)
        d = f32(f32(c - self.cos_total) / f32(self.cos_start - self.cos_total))
        return f32(f32(d * d) * f32(d * d))

    def sample_le(self, u0):
        """Sample_Le: (ray direction, Le, pdfDir); the origin is self.p, nLight = d, pdfPos = 1."""
        if self.kind == LIGHT_POINT:
            return uniform_sample_sphere(u0), self.I, INV_4PI
        d = xform_vec(self.l2w, uniform_sample_cone(u0, self.cos_total))
        fo = self.falloff(d)
        return d, tuple(f32(c * fo) for c in self.I), uniform_cone_pdf(self.cos_total)


def uniform_sample_sphere(u):  # sampling.cpp:98-103
    z = f32(f32(1) - f32(f32(2) * u[0]))
    t = f32(f32(1) - f32(z * z))
    r = f32(np.sqrt(t if f32(0) < t else f32(0)))
    phi = f32(f32(f32(2) * PI) * u[1])
    s, c = rp.sincosf(phi)
    return (f32(r * c), f32(r * s), z)


def uniform_cone_pdf(cos_max):  # sampling.cpp:132-134
    return f32(f32(1) / f32(f32(f32(2) * PI) * f32(f32(1) - cos_max)))


def uniform_sample_cone(u, cos_max):  # sampling.cpp:136-142
    ct = f32(f32(f32(1) - u[0]) + f32(u[0] * cos_max))
    st = f32(np.sqrt(f32(f32(1) - f32(ct * ct))))
    phi = f32(f32(u[1] * f32(2)) * PI)
    s, c = rp.sincosf(phi)
    return (f32(c * st), f32(s * st), ct)


def merged_order(emit_tris, orders, n_triangles=None):
    """scene.lights: [("delta", k) | ("tri", i)].  Delta light k comes before the area lights of the
    triangles with index >= orders[k]; equal orders keep their array order; area lights keep theirs."""
    out = []
    ks = sorted(range(len(orders)), key=lambda k: orders[k])  # stable
    j = 0
    for i in emit_tris:
        while j < len(ks) and orders[ks[j]] <= i:
            out.append(("delta", ks[j]))
            j += 1
        out.append(("tri", i))
    out.extend(("delta", k) for k in ks[j:])
    return out
