"""Distant lights and two-sided diffuse area lights of the pure-Python float32 restatement (test infrastructure),
each from the reference text, NOT from the HIP:
* DistantLight (src/lights/distant.cpp): the constructor's wLight = Normalize(LightToWorld(from - to)) (:43-47,
  94-102), Preprocess's Scene::WorldBound().BoundingSphere (src/lights/distant.h, src/core/geometry.h
  Bounds3::BoundingSphere), Power (:61-63), Sample_Le (:69-85) with ConcentricSampleDisk
  (src/core/sampling.cpp:113-133) and Sample_Li (:49-59);
* DiffuseAreaLight with twoSided (src/lights/diffuse.cpp): Power (:64-66), the side choice and remap of Sample_Le
  (:100-112), L (src/lights/diffuse.h: `(twoSided || Dot(intr.n, w) > 0) ? Lemit : 0`).
The walks are those of tests/refpy_passes_bsdf.py (a BSDF object per triangle); this module restates only what the
two light kinds touch: the emission of a photon (photonbeam.cpp:393-418), EstimateDirect's light-sampling half for
a distant light and its two halves for a two-sided triangle (src/core/integrator.cpp:108-214), and the isect.Le
term of the camera path (photonbeam.cpp:528-529).  Nothing in refpy_passes / refpy_passes_bsdf / refpy_lights is
edited.  A DistantLight has an empty MediumInterface (distant.cpp:45): its photons start in vacuum (medium -1).

Every float operation is done on numpy float32 scalars in the reference's order.
"""
from __future__ import annotations

import numpy as np

import refpy_camera as rc
import refpy_passes_bsdf as rpb
import refpy_specular as rs
from refpy_lights import LIGHT_SPOT, lum, xform_vec
from refpy_media import ONE3, med_tr
from refpy_passes import ZERO3, _count, pack_beams, pack_segments, visibility_tr
from refpy_photon import (INF, INV_PI, ONE_MINUS_EPS, PI, RNG, add, coordinate_system, cosine_hemisphere, dot, f32,
                          hit_tri, length, mul, mul3, normalize, offset_origin, sample_tri, sincosf, sub)

LIGHT_DISTANT = 3
EMIT_TWO_SIDED = 2
PI_OVER_4 = f32(0.78539816339744830961)
PI_OVER_2 = f32(1.57079632679489661923)
COUNTERS = rpb.COUNTERS + ("distant_lit", "distant_shadowed", "le_from_behind", "emit_front", "emit_back")


def new_stats():
    return {k: 0 for k in COUNTERS}


# ---------------- DistantLight ----------------
def distant_wlight(frm, to, m=None):
    """CreateDistantLight's dir = from - to (distant.cpp:98-101) through the constructor's
    Normalize(LightToWorld(wLight)) (:47; Transform::operator()(Vector3f), transform.h:236-242; Normalize and
    Vector3::operator/, geometry.h).  m: the 4x4 LightToWorld, rows of float32 (None: identity)."""
    d = sub(tuple(f32(x) for x in frm), tuple(f32(x) for x in to))
    if m is not None:
        d = xform_vec([[f32(v) for v in row] for row in m], d)
    return normalize(d)


def bounding_sphere(lo, hi):
    """Bounds3::BoundingSphere (geometry.h): center = (pMin + pMax) / 2 (Point3::operator/ multiplies by 1 / f),
    radius = Inside(center, *this) ? Distance(center, pMax) : 0."""
    inv = f32(f32(1) / f32(2))
    center = tuple(f32(inv * v) for v in add(lo, hi))
    inside = all(lo[k] <= center[k] <= hi[k] for k in range(3))
    return center, (length(sub(center, hi)) if inside else f32(0))


def concentric_sample_disk(ux, uy):
    """ConcentricSampleDisk, sampling.cpp:113-133."""
    ox, oy = f32(f32(f32(2) * ux) - f32(1)), f32(f32(f32(2) * uy) - f32(1))
    if ox == 0 and oy == 0:
        return f32(0), f32(0)
    if abs(ox) > abs(oy):
        r, theta = ox, f32(PI_OVER_4 * f32(oy / ox))
    else:
        r, theta = oy, f32(PI_OVER_2 - f32(PI_OVER_4 * f32(ox / oy)))
    s, c = sincosf(theta)
    return f32(r * c), f32(r * s)


class DistantLight:
    """A bre_light of type BRE_LIGHT_DISTANT as the DistantLight constructor leaves it: L in `I`, the world-space
    wLight in light_to_world[0..2].  preprocess() is DistantLight::Preprocess(scene)."""

    def __init__(self, L):
        self.kind = LIGHT_DISTANT
        self.I = tuple(f32(x) for x in L.I)
        self.w = tuple(f32(L.light_to_world[k]) for k in range(3))
        self.order = int(L.order)
        self.center, self.radius = (f32(0),) * 3, f32(0)

    def preprocess(self, lo, hi):
        self.center, self.radius = bounding_sphere(lo, hi)

    def power_y(self):  # L * Pi * worldRadius * worldRadius, distant.cpp:61-63
        return lum(tuple(f32(f32(f32(c * PI) * self.radius) * self.radius) for c in self.I))

    def sample_le(self, u):
        """distant.cpp:69-85: (origin, direction, Le, pdfPos, pdfDir); nLight = the direction; no SpawnRay."""
        v1, v2 = coordinate_system(self.w)
        cx, cy = concentric_sample_disk(*u)
        r = self.radius
        p_disk = add(self.center, mul(add(mul(v1, cx), mul(v2, cy)), r))
        o = add(p_disk, mul(self.w, r))
        with np.errstate(divide="ignore"):
            pdf_pos = f32(f32(1) / f32(f32(PI * r) * r))
        return o, tuple(-x for x in self.w), self.I, pdf_pos, f32(1)

    def sample_li(self, p):
        """distant.cpp:49-59: (wi, Li, pOutside); pdf = 1."""
        return self.w, self.I, add(p, mul(self.w, f32(f32(2) * self.radius)))


# ---------------- DiffuseAreaLight, twoSided ----------------
def two_sided_remap(u0):
    """diffuse.cpp:103-111: (remapped u[0], the far side was chosen)."""
    if u0 < f32(0.5):
        v = f32(u0 * f32(2))
        return (v if v < ONE_MINUS_EPS else ONE_MINUS_EPS), False
    v = f32(f32(u0 - f32(0.5)) * f32(2))
    return (v if v < ONE_MINUS_EPS else ONE_MINUS_EPS), True


def two_sided_direction(u):
    """diffuse.cpp:100-112: (w in the light's frame, pdfDir = 0.5f * CosineHemispherePdf(|w.z|))."""
    u0, far = two_sided_remap(u[0])
    w = list(cosine_hemisphere(u0, u[1]))
    if far:
        w[2] = f32(w[2] * f32(-1))
    return tuple(w), f32(f32(0.5) * f32(f32(abs(w[2])) * INV_PI))


def area_power_y(T, two_sided):
    """(twoSided ? 2 : 1) * Lemit * area * Pi, its y() (diffuse.cpp:64-66)."""
    k = f32(2) if two_sided else f32(1)
    return lum(tuple(f32(f32(f32(c * k) * T["area"]) * PI) for c in T["Le"]))


def area_L(sc, li, n, w):
    """DiffuseAreaLight::L(intr, w), diffuse.h."""
    return sc.tris[li]["Le"] if (li in sc.two_sided or dot(n, w) > 0) else ZERO3


class Scene(rpb.Scene):
    """refpy_passes_bsdf.Scene with DistantLight records among the delta lights and `two_sided`, the emitting
    triangles whose bre_triangle.emit is BRE_EMIT_TWO_SIDED; the power distribution is rebuilt over both
    (ComputeLightPowerDistribution, integrator.cpp:217-225; Distribution1D, sampling.h:57-69)."""

    def __init__(self, s, lights=(), *args, **kw):
        lights = list(lights)
        # the base class restates point and spot lights only: a distant light keeps its place in the order
        stand_in = []
        for L in lights:
            if L.type == LIGHT_DISTANT:
                P = type(L)()
                P.type, P.order = 1, L.order
                for i in range(4):
                    P.light_to_world[5 * i] = P.world_to_light[5 * i] = 1.0
                stand_in.append(P)
            else:
                stand_in.append(L)
        super().__init__(s, stand_in, *args, **kw)
        self.delta = [DistantLight(L) if L.type == LIGHT_DISTANT else d for L, d in zip(lights, self.delta)]
        self.two_sided = {i for i in self.lights if s.triangles[i].emit == EMIT_TWO_SIDED}
        # Scene::WorldBound(): the union of the triangles' bounds
        P = [v for t in self.tris for v in t["p"]]
        lo = tuple(min(v[k] for v in P) for k in range(3))
        hi = tuple(max(v[k] for v in P) for k in range(3))
        for i, d in enumerate(self.delta):
            if d.kind == LIGHT_DISTANT:
                d.preprocess(lo, hi)
                assert self.light_med[i] == -1 and not s.has_medium, "a distant light is in vacuum"
        func = [area_power_y(self.tris[i], i in self.two_sided) if kind == "tri" else self.delta[i].power_y()
                for kind, i in self.all_lights]
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


# ---------------- photon pass ----------------
def trace_photon(sc, seq, max_depth, radius, info=None, stats=None):
    """Beams of one photon (photonbeam.cpp:393-418): a light by power, its Sample_Le, the walk.  `info` receives
    the chosen light, its kind, and for a two-sided triangle the side the photon left on."""
    rng = RNG(seq)
    out = []
    ln, light_pdf = sc.sample_light(rng.uniform())
    u0 = rng.get2d()
    u1 = rng.get2d()
    rng.uniform()  # uLightTime
    kind, idx = sc.all_lights[ln]
    if info is not None:
        info.update(light=ln, kind=kind, falloff=None, side=None)
    if kind == "tri":
        L = sc.tris[idx]
        p, perr, nl, pdf_pos = sample_tri(L, *u0)
        if idx in sc.two_sided:
            wl, pdf_dir = two_sided_direction(u1)
            _count(stats, "emit_front" if wl[2] > 0 else "emit_back")
            if info is not None:
                info["side"] = "front" if wl[2] > 0 else "back"
        else:
            wl = cosine_hemisphere(*u1)
            pdf_dir = f32(wl[2] * INV_PI)
        v1, v2 = coordinate_system(nl)
        w = add(add(mul(v1, wl[0]), mul(v2, wl[1])), mul(nl, wl[2]))
        o = offset_origin(p, perr, nl, w)  # pShape.SpawnRay(w)
        Le = area_L(sc, idx, nl, w)
        inside, outside = sc.pair[idx]
        med = outside if dot(w, nl) > 0 else inside
    else:
        D = sc.delta[idx]
        if D.kind == LIGHT_DISTANT:
            o, w, Le, pdf_pos, pdf_dir = D.sample_le(u0)
            nl = w
            med = -1  # MediumInterface(): Ray(..., medium = nullptr)
        else:
            w, Le, pdf_dir = D.sample_le(u0)
            o, nl, pdf_pos = D.p, w, f32(1)
            med = sc.light_med[idx]
            if info is not None and D.kind == LIGHT_SPOT:
                info["falloff"] = D.falloff(w)
    if pdf_pos == 0 or pdf_dir == 0 or all(x == 0 for x in Le):
        return out
    ad = f32(abs(dot(nl, w)))
    den = f32(f32(light_pdf * pdf_pos) * pdf_dir)
    beta = tuple(f32(f32(ad * x) / den) for x in Le)
    if all(x == 0 for x in beta):
        return out
    if kind != "tri" and med != sc.cam_med:
        _count(stats, "delta_other_medium")
    rpb.walk(sc, rng, out, o, w, 0, beta, med, max_depth, radius, stats)
    return out


def trace_photons(sc, n_photons, iteration=0, max_depth=5, radius=0.01, first=None, infos=None, stats=None):
    """Photons [0, first or n_photons) of a pass of n_photons: the beams in order, and per photon their number."""
    beams, counts = [], []
    for i in range(first if first is not None else n_photons):
        info = {} if infos is not None else None
        b = trace_photon(sc, iteration * n_photons + i + 1, max_depth, radius, info, stats)
        if infos is not None:
            infos.append(info)
        counts.append(len(b))
        beams.extend(b)
    return pack_beams(beams, counts)


# ---------------- camera pass ----------------
def estimate_direct_distant(sc, smp, p, perr, q, bsdf, tri, med, wo, D, stats):
    """EstimateDirect with IsDeltaLight (integrator.cpp:108-165) over DistantLight::Sample_Li: the shadow ray runs
    to pOutside, an Interaction without a normal or an error bound (interaction.h:73-78)."""
    wi, Li, p_outside = D.sample_li(p)
    if rc.black(Li):
        return ZERO3
    ad = f32(abs(dot(wi, q["n"])))
    with np.errstate(all="ignore"):
        f = tuple(f32(x * ad) for x in bsdf.f(q, wo, wi, stats))
    if rc.black(f):
        return ZERO3
    Li = mul3(Li, visibility_tr(sc, smp, p, perr, tri, med, p_outside, ZERO3, ZERO3, stats))
    if rc.black(Li):
        _count(stats, "distant_shadowed")
        return ZERO3
    _count(stats, "distant_lit")
    return tuple(f32(f32(0) + f32(f32(a * b) / f32(1))) for a, b in zip(f, Li))


def estimate_direct_area(sc, smp, p, perr, q, bsdf, tri, med, wo, li, us, ul, stats):
    """EstimateDirect for the DiffuseAreaLight on triangle li, one- or two-sided, handleMedia = true
    (integrator.cpp:108-214; diffuse.cpp:68-87)."""
    L = sc.tris[li]
    Ld = [f32(0)] * 3
    sp, sperr, sn, light_pdf = sample_tri(L, *ul)
    w = sub(sp, p)
    if rc.lensq(w) == 0:
        light_pdf = f32(0)
    else:
        w = normalize(w)
        with np.errstate(divide="ignore"):
            light_pdf = f32(light_pdf * f32(rc.lensq(sub(p, sp)) / f32(abs(dot(sn, rc.neg(w))))))
        if np.isinf(light_pdf):
            light_pdf = f32(0)
    Li = ZERO3
    if light_pdf == 0 or rc.lensq(sub(sp, p)) == 0:
        light_pdf = f32(0)
    else:
        wi = normalize(sub(sp, p))
        Li = area_L(sc, li, sn, rc.neg(wi))  # L(pShape, -wi)
    if light_pdf > 0 and not rc.black(Li):
        ad = f32(abs(dot(wi, q["n"])))
        with np.errstate(all="ignore"):
            f = tuple(f32(x * ad) for x in bsdf.f(q, wo, wi, stats))
        scat_pdf = bsdf.pdf(q, wo, wi)
        if not rc.black(f):
            Li = mul3(Li, visibility_tr(sc, smp, p, perr, tri, med, sp, sperr, sn, stats))
            if not rc.black(Li):
                with np.errstate(all="ignore"):
                    wgt = rc.power_heuristic(light_pdf, scat_pdf)
                    Ld = [f32(Ld[c] + f32(f32(f32(f[c] * Li[c]) * wgt) / light_pdf)) for c in range(3)]
    bs = bsdf.sample(q, wo, us[0], us[1], rs.RADIANCE, stats, sc.normals)
    if bs is None:
        return tuple(Ld)
    wi, scat_pdf, f = bs[:3]
    ad = f32(abs(dot(wi, q["n"])))
    with np.errstate(all="ignore"):
        f = tuple(f32(x * ad) for x in f)
    if rc.black(f) or not scat_pdf > 0:
        return tuple(Ld)
    ro = offset_origin(p, perr, q["n"], wi)
    hl = hit_tri(L, ro, wi, INF)  # Shape::Pdf(ref, wi), shape.cpp:72-87
    if hl is None:
        return tuple(Ld)
    with np.errstate(divide="ignore"):
        light_pdf = f32(rc.lensq(sub(p, hl[1])) / f32(f32(abs(dot(L["n"], rc.neg(wi)))) * L["area"]))
    if np.isinf(light_pdf) or light_pdf == 0:
        return tuple(Ld)
    with np.errstate(all="ignore"):
        wgt = rc.power_heuristic(scat_pdf, light_pdf)
    m = sc.towards(tri, wi, med)
    tr = ONE3
    while True:  # Scene::IntersectTr
        found, tmax = sc.intersect(ro, wi)
        if m >= 0:
            tr = mul3(tr, med_tr(sc.media[m], smp, ro, wi, tmax))
        if found is None or not sc.iface[found[2]]:
            break
        hn = sc.tris[found[2]]["n"]
        ro = offset_origin(found[0], found[1], hn, wi)
        m = sc.towards(found[2], wi, m)
    if found is not None and found[2] == li:  # lightIsect.Le(-wi)
        Le = area_L(sc, li, L["n"], rc.neg(wi))
        if not rc.black(Le):
            with np.errstate(all="ignore"):
                Ld = [f32(Ld[c] + f32(f32(f32(f32(f[c] * Le[c]) * tr[c]) * wgt) / scat_pdf)) for c in range(3)]
    return tuple(Ld)


def camera_pass(sc, width, height, iteration=0, max_depth=5, render_surfaces=True, render_media=True, stats=None):
    """The camera paths of PhotonBeamIntegrator::Render (photonbeam.cpp:456-555): segments in row-major pixel
    order (path order within a pixel) + surface radiance (W*H, 3)."""
    cam = rc.Camera(sc.struct, width, height)
    halton = rc.LazyHalton(width, height)
    emit = set(sc.lights)
    nl = len(sc.all_lights)
    segs = []
    surface = np.zeros((width * height, 3), np.float32)
    for py in range(height):
        for px in range(width):
            smp = rc.AwesomeSampler(halton, halton.index(px, py, iteration), rc.good_pixel_index(width, height, px, py))
            fx, fy = smp.get2d()
            smp.get1d()  # time
            smp.get2d()  # lens (pinhole)
            o, d = cam.ray(f32(f32(px) + fx), f32(f32(py) + fy))
            beta = ONE3
            Ld = [f32(0)] * 3
            pixel = py * width + px
            specular_bounce = False
            med = sc.cam_med
            depth = ordinal = 0
            while depth < max_depth:
                hit, tmax = sc.intersect(o, d)
                if hit is None:
                    break  # Le(ray) of an area, delta or distant light is 0
                M = sc.of(med)
                mb = med_tr(M, smp, o, d, tmax)
                if M is None:
                    _count(stats, "vacuum_segment")
                if render_media:
                    segs.append((o, hit[0], d, tmax, pixel, ordinal))
                    ordinal += 1
                beta = mul3(beta, mb)
                tri = hit[2]
                q = sc.tris[tri]
                passed = sc.iface[tri]
                if passed:  # :515-517
                    _count(stats, "camera_pass")
                    o = offset_origin(hit[0], hit[1], q["n"], d)
                    med = sc.towards(tri, d, med)
                else:
                    if not render_surfaces:
                        break
                    bsdf = sc.bsdf[tri]
                    wo = rc.neg(d)
                    if (depth == 0 or specular_bounce) and tri in emit:  # isect.Le(wo)
                        Le = area_L(sc, tri, q["n"], wo)
                        if not dot(q["n"], wo) > 0 and not rc.black(Le):
                            _count(stats, "le_from_behind")
                        Ld = [f32(Ld[c] + f32(beta[c] * Le[c])) for c in range(3)]
                        if depth > 0:
                            _count(stats, "le_after_specular")
                    # UniformSampleOneLight (integrator.cpp:85-106): its three draws come whatever the material
                    ln = min(int(f32(smp.get1d() * f32(nl))), nl - 1)
                    light_pdf = f32(f32(1) / f32(nl))
                    ul = smp.get2d()
                    us = smp.get2d()
                    kind, idx = sc.all_lights[ln]
                    args = (sc, smp, hit[0], hit[1], q, bsdf, tri, med, normalize(wo))
                    if bsdf.none:
                        ed = ZERO3
                    elif bsdf.specular:
                        ed = ZERO3
                        _count(stats, "direct_early_out")
                    elif kind == "tri":
                        ed = estimate_direct_area(*args, idx, us, ul, stats)
                    elif sc.delta[idx].kind == LIGHT_DISTANT:
                        ed = estimate_direct_distant(*args, sc.delta[idx], stats)
                    else:
                        ed = rpb.estimate_direct_delta(*args, sc.delta[idx], stats)
                    Ld = [f32(Ld[c] + f32(beta[c] * f32(ed[c] / light_pdf))) for c in range(3)]
                    if depth < max_depth - 1:
                        ux, uy = smp.get2d()
                        if bsdf.none:
                            break
                        s = bsdf.sample(q, wo, ux, uy, rs.RADIANCE, stats, sc.normals)
                        if s is None:
                            break
                        wi, pdf, f, typ, branch = s
                        if pdf == 0 or rc.black(f):
                            break
                        specular_bounce = (typ & rs.BSDF_SPECULAR) != 0
                        ad = f32(abs(dot(wi, q["n"])))
                        with np.errstate(all="ignore"):
                            beta = tuple(f32(beta[c] * f32(f32(f[c] * ad) / pdf)) for c in range(3))
                        o = offset_origin(hit[0], hit[1], q["n"], wi)
                        d = wi
                        med = sc.towards(tri, wi, med)
                y = lum(beta)
                if y < f32(0.25):
                    cp = f32(1) if f32(1) < y else y
                    if smp.get1d() > cp:
                        if passed:
                            _count(stats, "camera_pass_roulette")
                        break
                    beta = tuple(f32(b / cp) for b in beta)
                if not passed:
                    depth += 1
            if render_surfaces:
                surface[pixel] += np.array(Ld, np.float32)
    return pack_segments(segs, surface)
