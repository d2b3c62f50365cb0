"""Pure-Python float32 restatement of the photon pass with point and spot lights (test infrastructure).

Built on refpy_photon's Scene, RNG, samplers and media.  New here, each from the reference text:
* the merged scene.lights order of delta lights and emitting triangles (api.cpp: lights are appended
  in declaration order; bre_light.order = triangles declared before the light);
* Power().y() of a PointLight (src/lights/point.cpp:55) and a SpotLight (src/lights/spot.cpp:75-77);
* PointLight::Sample_Le (point.cpp:61-71), SpotLight::Sample_Le and Falloff (spot.cpp:64-73, 83-93),
  UniformSampleSphere / UniformSampleCone / UniformConePdf (src/core/sampling.cpp:98-103, 132-142);
* the walk of TracePhotonBeamRecursive as a function (refpy_photon.trace_photon keeps it in a closure).
Every float operation is done on numpy float32 scalars in the reference's order.
"""
from __future__ import annotations

import numpy as np

import refpy_photon as rp
from refpy_photon import (INV_PI, PI, RNG, add, coordinate_system, cosine_hemisphere, dot, f32, grid_sample,
                          grid_tr, hg_sample, length, logf, mul, normalize, offset_origin)

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


class Scene(rp.Scene):
    """refpy_photon.Scene plus delta lights: self.all_lights is scene.lights in the reference's order,
    and lfunc / lcdf / lint its power distribution (ComputeLightPowerDistribution)."""

    def __init__(self, s, lights=()):
        with np.errstate(all="ignore"):  # a scene without an emitting triangle: 0 / 0 in the base class
            super().__init__(s)
        self.delta = [DeltaLight(L) for L in lights]
        self.all_lights = merged_order(self.lights, [d.order for d in self.delta])
        area_func = dict(zip(self.lights, self.lfunc))
        func = [area_func[i] if kind == "tri" else self.delta[i].power_y() for kind, i in self.all_lights]
        nl = len(func)
        cdf = [f32(0)] * (nl + 1)
        for i in range(1, nl + 1):
            cdf[i] = f32(cdf[i - 1] + f32(func[i - 1] / f32(nl)))
        fint = cdf[nl]
        if fint == 0:
            cdf = [f32(f32(i) / f32(nl)) for i in range(nl + 1)]
        else:
            cdf = [cdf[0]] + [f32(c / fint) for c in cdf[1:]]
        self.lfunc, self.lcdf, self.lint = func, cdf, fint


def walk(sc, rng, out, o, d, depth, beta, max_depth, radius):
    """TracePhotonBeamRecursive, photonbeam.cpp:258-325."""
    while depth < max_depth:
        hit, tmax = sc.intersect(o, d)
        if hit is None:
            return
        scattered = False
        if sc.medium and sc.grid:
            t = grid_sample(sc, rng, o, d, tmax)
            scattered = t is not None
        elif sc.medium:
            ch = min(int(f32(rng.uniform() * f32(3))), 2)
            dist = f32(-logf(f32(f32(1) - rng.uniform())) / sc.sigma_t[ch])
            dl = f32(dist * length(d))
            t = tmax if tmax < dl else dl
            scattered = bool(t < tmax)
        if all(x == 0 for x in beta):
            return
        if scattered:
            hx, hy = rng.get2d()
            wi = hg_sample(sc.g, tuple(-x for x in d), hx, hy)
            trv = (grid_tr(sc, rng, o, d, tmax),) * 3 if sc.grid else sc.tr(d, tmax)
            walk(sc, rng, out, add(o, mul(d, t)), wi, depth + 1, tuple(f32(b * x) for b, x in zip(beta, trv)),
                 max_depth, radius)
        if sc.medium and sc.grid:
            bm = (grid_tr(sc, rng, o, d, tmax),) * 3
        else:
            bm = sc.tr(d, tmax) if sc.medium else (f32(1),) * 3
        out.append((o, hit[0], f32(radius), tuple(f32(a * b) for a, b in zip(bm, beta))))
        q = sc.tris[hit[2]]
        ux, uy = rng.get2d()
        if all(x == 0 for x in q["kd"]):
            return
        wo = tuple(-x for x in d)
        woz = dot(wo, q["n"])
        if woz == 0:
            return
        wil = list(cosine_hemisphere(ux, uy))
        if woz < 0:
            wil[2] = f32(wil[2] * f32(-1))
        pdf = f32(abs(wil[2]) * INV_PI) if f32(woz * wil[2]) > 0 else f32(0)
        fr = tuple(f32(k * INV_PI) for k in q["kd"])
        if pdf == 0 or all(x == 0 for x in fr):
            return
        ss, ts, n = q["ss"], q["ts"], q["n"]
        wi = tuple(f32(f32(f32(ss[i] * wil[0]) + f32(ts[i] * wil[1])) + f32(n[i] * wil[2])) for i in range(3))
        adw = f32(abs(dot(wi, n)))
        bn = tuple(f32(f32(f32(f32(bm[c] * beta[c]) * fr[c]) * adw) / pdf) for c in range(3))
        o = offset_origin(hit[0], hit[1], n, wi)
        d = wi
        ratio = f32(f32(1) - f32(lum(bn) / lum(beta)))
        qrr = ratio if f32(0) < ratio else f32(0)
        if rng.uniform() < qrr:
            return
        beta = tuple(f32(x / f32(f32(1) - qrr)) for x in bn)
        depth += 1


def trace_photon(sc: Scene, seq: int, max_depth: int, radius: float, info=None):
    """Beams of one photon (photonbeam.cpp:393-418): a light by power, its Sample_Le, the walk.
    `info`, a dict, receives the chosen light and, for a spot, the emission's Falloff."""
    rng = RNG(seq)
    out = []
    ln, light_pdf = sc.sample_light(rng.uniform())
    u0 = rng.get2d()
    u1 = rng.get2d()
    rng.uniform()  # uLightTime
    kind, idx = sc.all_lights[ln]
    if info is not None:
        info.update(light=ln, kind=kind, falloff=None)
    if kind == "tri":
        L = sc.tris[idx]
        p, perr, nl, pdf_pos = sc.sample_tri(L, *u0)
        wl = cosine_hemisphere(*u1)
        pdf_dir = f32(wl[2] * INV_PI)
        v1, v2 = coordinate_system(nl)
        w = add(add(mul(v1, wl[0]), mul(v2, wl[1])), mul(nl, wl[2]))
        o = offset_origin(p, perr, nl, w)
        Le = L["Le"] if dot(nl, w) > 0 else (f32(0),) * 3
    else:
        D = sc.delta[idx]
        w, Le, pdf_dir = D.sample_le(u0)
        o, nl, pdf_pos = D.p, w, f32(1)
        if info is not None and D.kind == LIGHT_SPOT:
            info["falloff"] = D.falloff(w)
    if pdf_pos == 0 or pdf_dir == 0 or all(x == 0 for x in Le):
        return out
    ad = f32(abs(dot(nl, w)))
    den = f32(f32(light_pdf * pdf_pos) * pdf_dir)
    beta = tuple(f32(f32(ad * x) / den) for x in Le)
    if all(x == 0 for x in beta):
        return out
    walk(sc, rng, out, o, w, 0, beta, max_depth, radius)
    return out


def trace_photons(scene_struct, lights, n_photons, iteration=0, max_depth=5, radius=0.01, infos=None):
    """The whole pass (sequences iteration*N + i + 1), as refpy_photon.trace_photons returns it."""
    sc = Scene(scene_struct, lights)
    beams, counts = [], []
    for i in range(n_photons):
        info = {} if infos is not None else None
        b = trace_photon(sc, iteration * n_photons + i + 1, max_depth, radius, info)
        if infos is not None:
            infos.append(info)
        counts.append(len(b))
        beams.extend(b)
    n = len(beams)
    arr = {"start": np.zeros((n, 3), np.float32), "end": np.zeros((n, 3), np.float32),
           "radius": np.zeros(n, np.float32), "power": np.zeros((n, 3), np.float32)}
    for k, (s, e, r, pw) in enumerate(beams):
        arr["start"][k] = s
        arr["end"][k] = e
        arr["radius"][k] = r
        arr["power"][k] = pw
    arr["counts"] = np.array(counts, np.int32)
    return arr
