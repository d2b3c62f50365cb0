"""Pure-Python float32 restatement of the photon pass and the camera pass (test infrastructure): the expected
value of every bit-exact GPU test of the two passes, each function here exactly once.

Written from the reference text, NOT from oracle/, on the components beside it: refpy_photon (float32 math, RNG,
Halton, triangles, Henyey-Greenstein, the grid medium), refpy_lights (point and spot lights, the merged light
order), refpy_camera (camera, sampler, matte BSDF), refpy_specular (mirror and glass) and refpy_media (a medium).
* the photon pass: a light by power, its Sample_Le, TracePhotonBeamRecursive (src/integrators/photonbeam.cpp:
  258-325, 383-421), with the material's BSDF chosen per triangle (TransportMode::Importance);
* the camera path of PhotonBeamIntegrator::Render (:456-555): Scene::Intersect, UniformSampleOneLight /
  EstimateDirect (src/core/integrator.cpp:85-214) for diffuse area lights (with MIS) and for delta lights
  (Sample_Li of point.cpp:44-53 and spot.cpp:53-62, no MIS), specularBounce and the isect.Le term, EstimateDirect
  on a specular vertex (no shadow ray, no Tr draw), the bounce (TransportMode::Radiance) and the roulette;
* the medium a ray carries: Ray::medium, taken by Interaction::GetMedium at every spawn
  (src/core/interaction.h:64-88), with a surface hit's MediumInterface the primitive's own when it is a
  transition and MediumInterface(ray.medium) when not (GeometricPrimitive::Intersect, primitive.cpp:97-101);
  a ray in vacuum (a null Medium*) draws nothing and has Tr = 1;
* the start of a photon: DiffuseAreaLight::Sample_Le gives pShape its own mediumInterface (diffuse.cpp), a
  PointLight / SpotLight ray starts in mediumInterface.inside (point.cpp, spot.cpp); the camera ray in
  Camera::medium;
* a surface without a BSDF (Material "" / "none"): TracePhotonBeamRecursive pushes the beam, then
  `--depth; photonRay = isect.SpawnRay(photonRay.d); continue;` before its Get2D (photonbeam.cpp:290-304);
  the camera path records the segment, multiplies beta by the segment's Tr, passes through with the depth not
  counted and still runs the roulette (:489-517, 549-554);
* VisibilityTester::Tr as its loop (src/core/light.cpp:63-81) and Scene::IntersectTr (src/core/scene.cpp:62-75)
  in EstimateDirect with handleMedia.
A camera segment's "depth" is its ordinal along the pixel's path, which is the depth where no interface is crossed.

`stats`, a dict from new_stats(), counts the branches taken (COUNTERS).  Every float operation is done on numpy
float32 scalars in the reference's order.
"""
from __future__ import annotations

import numpy as np

import refpy_camera as rc
import refpy_specular as rs
from refpy_lights import LIGHT_SPOT, DeltaLight, lum, merged_order
from refpy_media import ONE3, Medium, med_sample, med_tr
from refpy_photon import (INF, INV_PI, PI, RNG, add, coordinate_system, cosine_hemisphere, cross, dot, f32, hg_sample,
                          hit_tri, length, mul, mul3, normalize, offset_origin, sample_tri, sub)

MATERIAL_COUNTERS = ("mirror_reflect", "glass_reflect", "transmit_enter", "transmit_leave", "tir", "refract_fail",
                     "le_after_specular", "direct_early_out")
MEDIA_COUNTERS = ("photon_pass", "camera_pass", "camera_pass_roulette", "vis_crossed", "vis_blocked_after_interface",
                  "intersect_tr_crossed", "vacuum_segment", "glass_medium_change", "delta_other_medium")
SHADOW_COUNTERS = ("shadow_blocked", "shadow_clear")
COUNTERS = MATERIAL_COUNTERS + MEDIA_COUNTERS + SHADOW_COUNTERS
ZERO3 = (f32(0),) * 3


def new_stats():
    return {k: 0 for k in COUNTERS}


def _count(stats, key):
    if stats is not None and key in stats:  # specular_sample's other branches ("wo_z0", "pdf0") are not counted
        stats[key] += 1


class Scene:
    """What a context holds when a pass runs: the bre_scene struct `s`, the delta lights, the material table and
    map (per triangle -1, its matte kd, or an entry) and, optionally, the media table with per triangle its
    (inside, outside) pair, the camera's medium and the delta lights'.  With a table the scene has no medium of
    its own.  Without one every ray is in the scene's own medium (has_medium 1 or 2: it fills all space), or in
    vacuum, and no triangle is a transition: the table then has that one entry, or none.

    self.all_lights is scene.lights in the reference's order, lfunc / lcdf / lint its power distribution.
    `exhaustive` makes intersect() test every triangle, as Scene::Intersect does, instead of filtering first."""

    def __init__(self, s, lights=(), materials=(), triangle_material=(), media=(), tri_inside=(), tri_outside=(),
                 camera_medium=-1, light_medium=(), exhaustive=False):
        self.struct = s
        self.exhaustive = exhaustive
        # one dict per pbrt Triangle (shapes/triangle.cpp)
        self.tris = []
        self.lights = []
        for i in range(s.n_triangles):
            t = s.triangles[i]
            p0, p1, p2 = (tuple(f32(x) for x in t.p[k]) for k in range(3))
            dp02, dp12 = sub(p0, p2), sub(p1, p2)
            # dpdu = (duv12[1] * dp02 - duv02[1] * dp12) * invdet with -1, -1, 1 (triangle.cpp:276-285)
            dpdu = mul(sub(mul(dp02, f32(-1)), mul(dp12, f32(-1))), f32(1))
            n = normalize(cross(dp02, dp12))
            ns = normalize(cross(sub(p1, p0), sub(p2, p0)))
            if t.flip:
                n = tuple(-x for x in n)
                ns = tuple(-x for x in ns)
            ss = normalize(dpdu)
            area = f32(0.5 * float(length(cross(sub(p1, p0), sub(p2, p0)))))
            self.tris.append(dict(p=(p0, p1, p2), n=n, ns=ns, ss=ss, ts=cross(n, ss), area=area,
                                  kd=tuple(f32(x) for x in t.kd), Le=tuple(f32(x) for x in t.Le)))
            if t.emit:
                self.lights.append(i)
        self.delta = [DeltaLight(L) for L in lights]
        self.all_lights = merged_order(self.lights, [d.order for d in self.delta])
        # ComputeLightPowerDistribution: a triangle's Power() = 1 * Lemit * area * Pi, its y() (diffuse.cpp:64-66)
        func = []
        for kind, i in self.all_lights:
            if kind == "tri":
                T = self.tris[i]
                func.append(lum(tuple(f32(f32(f32(c * f32(1)) * T["area"]) * PI) for c in T["Le"])))
            else:
                func.append(self.delta[i].power_y())
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
        # materials: per triangle None (its matte kd) or a Mat
        table = [rs.Mat.of(m) for m in materials]
        tm = list(triangle_material) if table else [-1] * len(self.tris)
        assert len(tm) == len(self.tris)
        self.mat = [None if k < 0 else table[k] for k in tm]
        self.iface = [m is not None and m.kind == rs.INTERFACE for m in self.mat]
        # media: the table, or the scene's own medium as a table of one that no triangle leaves
        if len(media):
            assert not s.has_medium
            self.media = [Medium(m) for m in media]
            self.pair = list(zip(tri_inside, tri_outside))
            self.cam_med = int(camera_medium)
            self.light_med = [int(x) for x in light_medium]
        else:
            self.media = [Medium(s, s.has_medium)] if s.has_medium else []
            own = len(self.media) - 1  # 0, or -1: vacuum
            self.pair = [(own, own)] * len(self.tris)
            self.cam_med = own
            self.light_med = [own] * len(self.delta)
        assert len(self.pair) == len(self.tris) and len(self.light_med) == len(self.delta)
        # for intersect's candidate filter, in double: a vertex, the plane normal and the bounds of each triangle
        P = np.array([[[float(c) for c in v] for v in t["p"]] for t in self.tris])
        self._p0 = P[:, 0]
        self._nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        self._lo, self._hi = P.min(axis=1) - 1e-3, P.max(axis=1) + 1e-3

    def sample_light(self, u):
        """Distribution1D::SampleDiscrete (sampling.h:90-100) with FindInterval (pbrt.h:377-389)."""
        size = len(self.lcdf)
        first, ln = 0, size
        while ln > 0:
            half = ln >> 1
            mid = first + half
            if self.lcdf[mid] <= u:
                first = mid + 1
                ln -= half + 1
            else:
                ln = half
        off = min(max(first - 1, 0), size - 2)
        pdf = f32(self.lfunc[off] / f32(self.lint * f32(len(self.lfunc)))) if self.lint > 0 else f32(0)
        return off, pdf

    def intersect(self, o, d, tmax=INF):
        """Scene::Intersect against ray.tMax: ((p, pError, triangle) or None, tMax).
        Triangle::Intersect runs, in scene order, only on the triangles the ray can hit at all: those whose plane
        it meets, in double, within 1e-3 of the triangle's bounds (the scenes are of unit size, float32 moves a
        hit by about 1e-7) or is nearly parallel to.  The others would return no hit, so the result is the same;
        tests/test_refpy_golden.py holds it to intersect_exhaustive on whole passes."""
        if self.exhaustive:
            return self.intersect_exhaustive(o, d, tmax)
        o64, d64 = np.array(o, np.float64), np.array(d, np.float64)
        den = self._nrm @ d64
        with np.errstate(all="ignore"):
            t = ((self._p0 - o64) * self._nrm).sum(axis=1) / den
            hit = o64 + t[:, None] * d64
            near = ((hit >= self._lo) & (hit <= self._hi)).all(axis=1) & (t > -1e-3)
        steep = np.abs(den) > 1e-9 * np.linalg.norm(self._nrm, axis=1) * np.linalg.norm(d64)
        best = None
        for i in np.nonzero(near | ~steep)[0]:
            h = hit_tri(self.tris[i], o, d, tmax)
            if h is None:
                continue
            tmax = h[0]
            best = (h[1], h[2], int(i))
        return best, tmax

    def intersect_exhaustive(self, o, d, tmax=INF):
        """Scene::Intersect as the reference runs it: every triangle, in scene order."""
        best = None
        for i, T in enumerate(self.tris):
            h = hit_tri(T, o, d, tmax)
            if h is None:
                continue
            tmax = h[0]
            best = (h[1], h[2], i)
        return best, tmax

    def of(self, med):
        return self.media[med] if med >= 0 else None

    def towards(self, tri, w, med):
        """GetMedium(w) at a point of triangle `tri` reached by a ray in medium `med`."""
        inside, outside = self.pair[tri]
        if inside == outside:
            return med
        return outside if dot(w, self.tris[tri]["n"]) > 0 else inside


# ---------------- photon pass ----------------
def walk(sc, rng, out, o, d, depth, beta, med, max_depth, radius, stats=None):
    """TracePhotonBeamRecursive, photonbeam.cpp:258-325, with the material's BSDF at :296-323."""
    while depth < max_depth:
        hit, tmax = sc.intersect(o, d)
        if hit is None:
            return
        M = sc.of(med)
        t = med_sample(M, rng, o, d, tmax)
        if all(x == 0 for x in beta):
            return
        if t is not None:
            hx, hy = rng.get2d()
            wi = hg_sample(M.g, tuple(-x for x in d), hx, hy)
            trv = med_tr(M, rng, o, d, tmax)
            walk(sc, rng, out, add(o, mul(d, t)), wi, depth + 1, mul3(beta, trv), med, max_depth, radius, stats)
        bm = med_tr(M, rng, o, d, tmax)
        if M is None:
            _count(stats, "vacuum_segment")
        out.append((o, hit[0], f32(radius), mul3(bm, beta)))
        tri = hit[2]
        q = sc.tris[tri]
        if sc.iface[tri]:  # :300-304, before the Get2D; beta is not multiplied by bm, no roulette
            _count(stats, "photon_pass")
            o = offset_origin(hit[0], hit[1], q["n"], d)
            med = sc.towards(tri, d, med)
            continue
        m = sc.mat[tri]
        ux, uy = rng.get2d()  # drawn before anything is known about the material (:313)
        wo = tuple(-x for x in d)
        branch = None
        if m is None:
            if all(x == 0 for x in q["kd"]):
                return
            woz = dot(wo, q["n"])
            if woz == 0:
                return
            wil = list(cosine_hemisphere(ux, uy))
            if woz < 0:
                wil[2] = f32(wil[2] * f32(-1))
            pdf = f32(abs(wil[2]) * INV_PI) if f32(woz * wil[2]) > 0 else f32(0)
            fr = tuple(f32(k * INV_PI) for k in q["kd"])
        else:
            if m.none:
                return  # matchingComps == 0
            wil, pdf, fr, _, branch = rs.specular_sample(m, rc.to_local(q, wo), ux, rs.IMPORTANCE)
            _count(stats, branch)
        if pdf == 0 or all(x == 0 for x in fr):
            return
        n = q["n"]
        wi = rs.to_world(q, wil)
        adw = f32(abs(dot(wi, n)))
        bn = tuple(f32(f32(f32(f32(bm[c] * beta[c]) * fr[c]) * adw) / pdf) for c in range(3))
        o = offset_origin(hit[0], hit[1], n, wi)
        d = wi
        new_med = sc.towards(tri, wi, med)
        ratio = f32(f32(1) - f32(lum(bn) / lum(beta)))
        qrr = ratio if f32(0) < ratio else f32(0)
        if rng.uniform() < qrr:
            return
        if new_med != med and branch in ("transmit_enter", "transmit_leave"):
            _count(stats, "glass_medium_change")
        med = new_med
        beta = tuple(f32(x / f32(f32(1) - qrr)) for x in bn)
        depth += 1


def trace_photon(sc, seq, max_depth, radius, info=None, stats=None):
    """Beams of one photon (photonbeam.cpp:393-418), in the reference's push order: a light by power, its
    Sample_Le, the walk; a list of (start, end, radius, power).  `info`, a dict, receives the chosen light and,
    for a spot, the emission's Falloff."""
    rng = RNG(seq)
    out = []
    ln, light_pdf = sc.sample_light(rng.uniform())  # lightDistr->SampleDiscrete
    u0 = rng.get2d()
    u1 = rng.get2d()
    rng.uniform()  # uLightTime
    kind, idx = sc.all_lights[ln]
    if info is not None:
        info.update(light=ln, kind=kind, falloff=None)
    if kind == "tri":
        L = sc.tris[idx]
        p, perr, nl, pdf_pos = sample_tri(L, *u0)
        wl = cosine_hemisphere(*u1)
        pdf_dir = f32(wl[2] * INV_PI)
        v1, v2 = coordinate_system(nl)
        w = add(add(mul(v1, wl[0]), mul(v2, wl[1])), mul(nl, wl[2]))
        o = offset_origin(p, perr, nl, w)
        Le = L["Le"] if dot(nl, w) > 0 else ZERO3
        inside, outside = sc.pair[idx]  # pShape.mediumInterface = mediumInterface; pShape.SpawnRay(w)
        med = outside if dot(w, nl) > 0 else inside
    else:
        D = sc.delta[idx]
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
    walk(sc, rng, out, o, w, 0, beta, med, max_depth, radius, stats)
    return out


def pack_beams(beams, counts):
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


def trace_photons(sc, n_photons, iteration=0, max_depth=5, radius=0.01, first=None, infos=None, stats=None):
    """Photons [0, first or n_photons) of a pass of n_photons (sequences iteration*N + i + 1): the beams in
    order, and per photon their number.  `infos`, a list, receives one trace_photon info per photon."""
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
def visibility_tr(sc, smp, p, perr, tri, med, tp, terr, tn, stats):
    """VisibilityTester::Tr (light.cpp:63-81) from the vertex (p, pError) on triangle `tri`, reached in medium
    `med`, to the light sample (tp, terr, tn), over Interaction::SpawnRayTo (interaction.h:73-78)."""
    ro = offset_origin(p, perr, sc.tris[tri]["n"], sub(tp, p))
    target = offset_origin(tp, terr, tn, sub(ro, tp))
    rd = sub(target, ro)
    m = sc.towards(tri, rd, med)
    Tr = ONE3
    crossed = 0
    while True:
        hit, tmax = sc.intersect(ro, rd, f32(f32(1) - f32(0.0001)))
        if hit is not None and not sc.iface[hit[2]]:
            _count(stats, "shadow_blocked")
            if crossed:
                _count(stats, "vis_blocked_after_interface")
            return ZERO3  # before any Tr draw of this segment
        if m >= 0:
            Tr = mul3(Tr, med_tr(sc.media[m], smp, ro, rd, tmax))
        if hit is None:
            break
        crossed += 1
        hn = sc.tris[hit[2]]["n"]
        ro = offset_origin(hit[0], hit[1], hn, sub(tp, hit[0]))
        target = offset_origin(tp, terr, tn, sub(ro, tp))
        rd = sub(target, ro)
        m = sc.towards(hit[2], rd, m)
    _count(stats, "shadow_clear")
    if crossed:
        _count(stats, "vis_crossed")
    return Tr


def estimate_direct_delta(sc, smp, p, perr, q, tri, med, wo, D, stats):
    """EstimateDirect with IsDeltaLight (integrator.cpp:108-165): no MIS weight, no BSDF-sampling half."""
    wi = normalize(sub(D.p, p))  # Sample_Li: point.cpp:44-53, spot.cpp:53-62
    fo = D.falloff(rc.neg(wi))
    dist2 = rc.lensq(sub(D.p, p))
    Li = tuple(f32(f32(c * fo) / dist2) for c in D.I)
    if rc.black(Li):
        return ZERO3
    ad = f32(abs(dot(wi, q["n"])))
    f = tuple(f32(x * ad) for x in rc.bsdf_f(q, wo, wi))
    if rc.black(f):
        return ZERO3
    Li = mul3(Li, visibility_tr(sc, smp, p, perr, tri, med, D.p, ZERO3, ZERO3, stats))
    if rc.black(Li):
        return ZERO3
    return tuple(f32(f32(0) + f32(f32(a * b) / f32(1))) for a, b in zip(f, Li))


def estimate_direct_area(sc, smp, p, perr, q, tri, med, wo, li, us, ul, stats):
    """EstimateDirect for the DiffuseAreaLight on triangle li, handleMedia = true (integrator.cpp:108-214)."""
    L = sc.tris[li]
    Ld = [f32(0)] * 3
    sp, sperr, sn, light_pdf = sample_tri(L, *ul)  # Shape::Sample(ref, u), shape.cpp:56-70
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
        if dot(sn, rc.neg(wi)) > 0:  # DiffuseAreaLight::L, one-sided
            Li = L["Le"]
    if light_pdf > 0 and not rc.black(Li):
        ad = f32(abs(dot(wi, q["n"])))
        f = tuple(f32(x * ad) for x in rc.bsdf_f(q, wo, wi))
        scat_pdf = rc.bsdf_pdf(q, wo, wi)
        if not rc.black(f):
            Li = mul3(Li, visibility_tr(sc, smp, p, perr, tri, med, sp, sperr, sn, stats))
            if not rc.black(Li):
                wgt = rc.power_heuristic(light_pdf, scat_pdf)
                Ld = [f32(Ld[c] + f32(f32(f32(f[c] * Li[c]) * wgt) / light_pdf)) for c in range(3)]
    bs = rc.bsdf_sample(q, wo, *us)
    if bs is None:
        return tuple(Ld)
    wi, scat_pdf, f = bs
    ad = f32(abs(dot(wi, q["n"])))
    f = tuple(f32(x * ad) for x in f)
    if rc.black(f) or not scat_pdf > 0:
        return tuple(Ld)
    ro = offset_origin(p, perr, q["n"], wi)
    hl = hit_tri(L, ro, wi, INF)  # Shape::Pdf(ref, wi), shape.cpp:72-87: this triangle alone
    if hl is None:
        return tuple(Ld)
    with np.errstate(divide="ignore"):
        light_pdf = f32(rc.lensq(sub(p, hl[1])) / f32(f32(abs(dot(L["n"], rc.neg(wi)))) * L["area"]))
    if np.isinf(light_pdf) or light_pdf == 0:
        return tuple(Ld)
    wgt = rc.power_heuristic(scat_pdf, light_pdf)
    # Scene::IntersectTr of it.SpawnRay(wi)
    m = sc.towards(tri, wi, med)
    tr = ONE3
    crossed = 0
    while True:
        found, tmax = sc.intersect(ro, wi)
        if m >= 0:
            tr = mul3(tr, med_tr(sc.media[m], smp, ro, wi, tmax))
        if found is None or not sc.iface[found[2]]:
            break
        crossed += 1
        hn = sc.tris[found[2]]["n"]
        ro = offset_origin(found[0], found[1], hn, wi)
        m = sc.towards(found[2], wi, m)
    if crossed:
        _count(stats, "intersect_tr_crossed")
    if found is not None and found[2] == li and dot(L["n"], rc.neg(wi)) > 0 and not rc.black(L["Le"]):
        Ld = [f32(Ld[c] + f32(f32(f32(f32(f[c] * L["Le"][c]) * tr[c]) * wgt) / scat_pdf)) for c in range(3)]
    return tuple(Ld)


def pack_segments(segs, surface):
    n = len(segs)
    out = {"o": np.zeros((n, 3), np.float32), "p": np.zeros((n, 3), np.float32), "d": np.zeros((n, 3), np.float32),
           "tmax": np.zeros(n, np.float32), "pixel": np.zeros(n, np.int32), "depth": np.zeros(n, np.int32)}
    for k, (o, p, d, t, pix, dep) in enumerate(segs):
        out["o"][k], out["p"][k], out["d"][k], out["tmax"][k], out["pixel"][k], out["depth"][k] = o, p, d, t, pix, dep
    out["surface"] = surface
    return out


def camera_pass(sc, width, height, iteration=0, max_depth=5, render_surfaces=True, render_media=True, stats=None):
    """The camera paths of PhotonBeamIntegrator::Render (photonbeam.cpp:456-555): segments in row-major pixel
    order (path order within a pixel) + surface radiance (W*H, 3), as oracle.camera_pass returns them."""
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
                    break  # area and delta lights: Le(ray) = 0
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
                if passed:  # :515-517: ray = isect.SpawnRay(ray.d); --depth
                    _count(stats, "camera_pass")
                    o = offset_origin(hit[0], hit[1], q["n"], d)
                    med = sc.towards(tri, d, med)
                else:
                    if not render_surfaces:
                        break
                    m = sc.mat[tri]
                    if m is not None and m.none:  # a BSDF without a BxDF: as a black kd
                        q = dict(q, kd=ZERO3)
                        m = None
                    wo = rc.neg(d)
                    if (depth == 0 or specular_bounce) and tri in emit and dot(q["n"], wo) > 0:  # isect.Le(wo)
                        Ld = [f32(Ld[c] + f32(beta[c] * q["Le"][c])) for c in range(3)]
                        if depth > 0:
                            _count(stats, "le_after_specular")
                    # UniformSampleOneLight (integrator.cpp:85-106): its three draws come whatever the material
                    ln = min(int(f32(smp.get1d() * f32(nl))), nl - 1)
                    light_pdf = f32(f32(1) / f32(nl))
                    ul = smp.get2d()
                    us = smp.get2d()
                    kind, idx = sc.all_lights[ln]
                    if m is not None:
                        # EstimateDirect with bsdfFlags = BSDF_ALL & ~BSDF_SPECULAR on a specular vertex: f = 0,
                        # no shadow ray, no Tr draw; the BSDF-sampling half has matchingComps == 0
                        ed = ZERO3
                        _count(stats, "direct_early_out")
                    elif kind == "tri":
                        ed = estimate_direct_area(sc, smp, hit[0], hit[1], q, tri, med, normalize(wo), idx, us, ul, stats)
                    else:
                        ed = estimate_direct_delta(sc, smp, hit[0], hit[1], q, tri, med, normalize(wo), sc.delta[idx],
                                                   stats)
                    Ld = [f32(Ld[c] + f32(beta[c] * f32(ed[c] / light_pdf))) for c in range(3)]
                    if depth < max_depth - 1:
                        ux, uy = smp.get2d()
                        branch = None
                        if m is None:
                            bs = rc.bsdf_sample(q, wo, ux, uy)
                            if bs is None or rc.black(bs[2]):
                                break
                            wi, pdf, f = bs
                            specular_bounce = False
                        else:
                            wil, pdf, f, typ, branch = rs.specular_sample(m, rc.to_local(q, wo), ux, rs.RADIANCE)
                            _count(stats, branch)
                            if pdf == 0 or rc.black(f):
                                break
                            wi = rs.to_world(q, wil)
                            specular_bounce = (typ & rs.BSDF_SPECULAR) != 0
                        ad = f32(abs(dot(wi, q["n"])))
                        beta = tuple(f32(beta[c] * f32(f32(f[c] * ad) / pdf)) for c in range(3))
                        o = offset_origin(hit[0], hit[1], q["n"], wi)
                        d = wi
                        new_med = sc.towards(tri, wi, med)
                        if new_med != med and branch in ("transmit_enter", "transmit_leave"):
                            _count(stats, "glass_medium_change")
                        med = new_med
                y = lum(beta)
                if y < f32(0.25):
                    cp = f32(1) if f32(1) < y else y  # std::min((Float)1, beta.y())
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
