"""The two walks of tests/refpy_passes.py with a BSDF object per triangle (test infrastructure): the photon pass and
the camera pass over every material, the old ones (a triangle's own matte kd, mirror, glass, interface) and the new
ones (plastic, metal, matte with sigma; tests/refpy_bsdf.py).

refpy_passes.py chooses between the Lambertian lobe and the specular one by hand in its loops; the reference does
not: both walks call ComputeScatteringFunctions and BSDF::Sample_f(..., BSDF_ALL) on whatever the ray hits
(src/integrators/photonbeam.cpp:296-323, 512-554) and EstimateDirect calls BSDF::f and BSDF::Pdf
(src/core/integrator.cpp:108-214).  This module restates only those loops and the two EstimateDirect functions,
over objects with f / pdf / sample; Scene, visibility_tr, the medium helpers and the packers are refpy_passes's.
The two modules are to be merged by a later change that may edit test helpers;
tests/test_glossy_refpy.py holds this one to refpy_passes bit for bit on the existing scenes.
"""
from __future__ import annotations

import numpy as np

import refpy_bsdf as rb
import refpy_camera as rc
import refpy_passes as rpass
import refpy_specular as rs
from refpy_lights import LIGHT_SPOT, lum
from refpy_media import ONE3, med_sample, med_tr
from refpy_passes import ZERO3, _count, pack_beams, pack_segments, visibility_tr
from refpy_photon import (INF, INV_PI, RNG, add, coordinate_system, cosine_hemisphere, dot, f32, hg_sample, hit_tri,
                          mul, mul3, normalize, offset_origin, sample_tri, sub)

COUNTERS = rpass.COUNTERS + rb.COUNTERS


def new_stats():
    return {k: 0 for k in COUNTERS}


# ---- a triangle's BSDF: `none` (no BxDF), `specular` (only specular lobes: BSDF::f and Pdf match nothing under
# BSDF_ALL & ~BSDF_SPECULAR), f, pdf, and sample -> (wi world, pdf, f, type, branch) or None where Sample_f's f is 0
# before anything is known ----
class MatteBsdf:
    """MatteMaterial with sigma 0 on the triangle's own kd: one LambertianReflection."""
    specular = False

    def __init__(self, q):
        self.none = all(x == 0 for x in q["kd"])

    def f(self, q, wo, wi, stats=None):
        return rc.bsdf_f(q, wo, wi)

    def pdf(self, q, wo, wi):
        return rc.bsdf_pdf(q, wo, wi)

    def sample(self, q, wo, u0, u1, mode, stats=None, normals=None):
        bs = rc.bsdf_sample(q, wo, u0, u1)
        if bs is None:
            return None
        return bs[0], bs[1], bs[2], rb.BSDF_REFLECTION | rb.BSDF_DIFFUSE, None


class SpecularBsdf:
    """MirrorMaterial / GlassMaterial with zero roughness: one specular lobe (refpy_specular)."""
    specular = True

    def __init__(self, m):
        self.m = m
        self.none = m.none

    def f(self, q, wo, wi, stats=None):
        return ZERO3

    def pdf(self, q, wo, wi):
        return f32(0)

    def sample(self, q, wo, u0, u1, mode, stats=None, normals=None):
        wil, pdf, f, typ, branch = rs.specular_sample(self.m, rc.to_local(q, wo), u0, mode)
        _count(stats, branch)
        if pdf == 0:
            return None
        return rs.to_world(q, wil), pdf, f, typ, branch


class GlossyBsdf:
    """Plastic, metal, matte with sigma: refpy_bsdf.Bsdf."""
    specular = False

    def __init__(self, b):
        self.b = b
        self.none = b.none

    def f(self, q, wo, wi, stats=None):
        return self.b.f(q, wo, wi, stats)

    def pdf(self, q, wo, wi):
        return self.b.pdf(q, wo, wi)

    def sample(self, q, wo, u0, u1, mode, stats=None, normals=None):
        s = self.b.sample(q, wo, u0, u1, stats, normals)
        return None if s is None else s + (None,)


class Scene(rpass.Scene):
    """refpy_passes.Scene plus self.bsdf, one object per triangle (None for an interface triangle); self.normals
    collects the (r, phi) of every normal-incidence microfacet sample of the passes run on it."""

    def __init__(self, s, lights=(), materials=(), triangle_material=(), *media_args, **kw):
        super().__init__(s, lights, materials, triangle_material, *media_args, **kw)
        table = []
        for m in materials:
            if m.type >= rb.MATTE:
                table.append(GlossyBsdf(rb.Bsdf.of(m)))
            elif m.type == rs.INTERFACE:
                table.append(None)
            else:
                table.append(SpecularBsdf(rs.Mat.of(m)))
        tm = list(triangle_material) if table else [-1] * len(self.tris)
        self.bsdf = [MatteBsdf(self.tris[i]) if k < 0 else table[k] for i, k in enumerate(tm)]
        self.normals = []


# ---------------- photon pass ----------------
def walk(sc, rng, out, o, d, depth, beta, med, max_depth, radius, stats=None):
    """TracePhotonBeamRecursive, photonbeam.cpp:258-325: BSDF::Sample_f of whatever material was hit."""
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
        bsdf = sc.bsdf[tri]
        ux, uy = rng.get2d()  # :313
        wo = tuple(-x for x in d)
        if bsdf.none:
            return  # matchingComps == 0
        s = bsdf.sample(q, wo, ux, uy, rs.IMPORTANCE, stats, sc.normals)
        if s is None:
            return
        wi, pdf, fr, _, branch = s
        if pdf == 0 or all(x == 0 for x in fr):
            return
        n = q["n"]
        adw = f32(abs(dot(wi, n)))
        with np.errstate(all="ignore"):
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
    """Beams of one photon (photonbeam.cpp:393-418): a light by power, its Sample_Le, the walk."""
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
        p, perr, nl, pdf_pos = sample_tri(L, *u0)
        wl = cosine_hemisphere(*u1)
        pdf_dir = f32(wl[2] * INV_PI)
        v1, v2 = coordinate_system(nl)
        w = add(add(mul(v1, wl[0]), mul(v2, wl[1])), mul(nl, wl[2]))
        o = offset_origin(p, perr, nl, w)
        Le = L["Le"] if dot(nl, w) > 0 else ZERO3
        inside, outside = sc.pair[idx]
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
def estimate_direct_delta(sc, smp, p, perr, q, bsdf, tri, med, wo, D, stats):
    """EstimateDirect with IsDeltaLight (integrator.cpp:108-165): no MIS weight, no BSDF-sampling half."""
    wi = normalize(sub(D.p, p))
    fo = D.falloff(rc.neg(wi))
    dist2 = rc.lensq(sub(D.p, p))
    Li = tuple(f32(f32(c * fo) / dist2) for c in D.I)
    if rc.black(Li):
        return ZERO3
    ad = f32(abs(dot(wi, q["n"])))
    with np.errstate(all="ignore"):
        f = tuple(f32(x * ad) for x in bsdf.f(q, wo, wi, stats))
    if rc.black(f):
        return ZERO3
    Li = mul3(Li, visibility_tr(sc, smp, p, perr, tri, med, D.p, ZERO3, ZERO3, stats))
    if rc.black(Li):
        return ZERO3
    return tuple(f32(f32(0) + f32(f32(a * b) / f32(1))) for a, b in zip(f, Li))


def estimate_direct_area(sc, smp, p, perr, q, bsdf, tri, med, wo, li, us, ul, stats):
    """EstimateDirect for the DiffuseAreaLight on triangle li, handleMedia = true (integrator.cpp:108-214)."""
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
        if dot(sn, rc.neg(wi)) > 0:
            Li = L["Le"]
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
    hl = hit_tri(L, ro, wi, INF)
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
        with np.errstate(all="ignore"):
            Ld = [f32(Ld[c] + f32(f32(f32(f32(f[c] * L["Le"][c]) * tr[c]) * wgt) / scat_pdf)) for c in range(3)]
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
                    break
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
                    if bsdf.none:
                        ed = ZERO3  # no BxDF: f = 0, and Sample_f has matchingComps == 0; nothing is drawn
                    elif bsdf.specular:
                        ed = ZERO3  # f = 0: no shadow ray, no Tr draw; the BSDF-sampling half matches no lobe
                        _count(stats, "direct_early_out")
                    elif kind == "tri":
                        ed = estimate_direct_area(sc, smp, hit[0], hit[1], q, bsdf, tri, med, normalize(wo), idx, us, ul,
                                                  stats)
                    else:
                        ed = estimate_direct_delta(sc, smp, hit[0], hit[1], q, bsdf, tri, med, normalize(wo),
                                                   sc.delta[idx], stats)
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
                        new_med = sc.towards(tri, wi, med)
                        if new_med != med and branch in ("transmit_enter", "transmit_leave"):
                            _count(stats, "glass_medium_change")
                        med = new_med
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
