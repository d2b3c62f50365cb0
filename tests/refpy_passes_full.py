"""The two walks over rough glass, uber, translucent and substrate surfaces (test infrastructure), on top of
tests/refpy_distant.py and tests/refpy_passes_bsdf.py without editing them, from the reference text, NOT from the HIP.

Both walks call BSDF::Sample_f(..., BSDF_ALL) on whatever the ray hits (src/integrators/photonbeam.cpp:296-323 in
TransportMode::Importance, :512-554 in Radiance), and EstimateDirect evaluates BSDF::f and Pdf and samples the BSDF
with bsdfFlags = BSDF_ALL & ~BSDF_SPECULAR (src/core/integrator.cpp:112-113, 135-137, 170-175).  For the materials
before these the two flag sets chose the same lobes, so the earlier modules carry no flags.  Here a BSDF holds
specular and non-specular, reflecting and transmitting lobes at once (tests/refpy_bsdf_full.py), so this module
restates:
* the photon walk (photonbeam.cpp:258-325) and a photon's emission as refpy_distant.trace_photon has it, to tag every
  beam with the BxDFType of the surface bounce that spawned its ray (0: emission, a medium scattering, an interface);
* the camera walk (photonbeam.cpp:456-555) as refpy_distant.camera_pass has it, handing EstimateDirect the
  non-specular view of the BSDF and recording per pixel what the non-vacuity conditions of the GPU tests need.
refpy_distant's estimate_direct_* functions are used as they are: they call f / pdf / sample on the view they are given.
"""
from __future__ import annotations

import numpy as np

import refpy_bsdf as rb
import refpy_bsdf_full as rf
import refpy_camera as rc
import refpy_distant as rd
import refpy_passes_bsdf as rpb
import refpy_specular as rs
from refpy_lights import lum
from refpy_media import ONE3, med_sample, med_tr
from refpy_passes import ZERO3, _count, pack_beams, pack_segments
from refpy_photon import (INV_PI, RNG, add, coordinate_system, cosine_hemisphere, dot, f32, hg_sample, mul, mul3,
                          normalize, offset_origin, sample_tri)

COUNTERS = rd.COUNTERS + rf.COUNTERS[len(rb.COUNTERS):] + (
    "direct_no_matching_lobe", "direct_transmitted_light", "photon_transmitted", "photon_uber_specular",
    "camera_transmitted", "camera_uber_specular")


def new_stats():
    return {k: 0 for k in COUNTERS}


class _DirectView:
    """The BSDF as EstimateDirect sees it: bsdfFlags = BSDF_ALL & ~BSDF_SPECULAR, TransportMode::Radiance."""

    def __init__(self, b):
        self.b = b

    def f(self, q, wo, wi, stats=None):
        f = self.b.f(q, wo, wi, rf.BSDF_NON_SPECULAR, rf.RADIANCE)
        if not rc.black(f) and not f32(dot(wi, q["n"]) * dot(wo, q["n"])) > 0:
            _count(stats, "direct_transmitted_light")
        return f

    def pdf(self, q, wo, wi):
        return self.b.pdf(q, wo, wi, rf.BSDF_NON_SPECULAR)

    def sample(self, q, wo, u0, u1, mode, stats=None, normals=None):
        s = self.b.sample(q, wo, u0, u1, rf.BSDF_NON_SPECULAR, rf.RADIANCE, stats, normals)
        return None if s is None else s + (None,)


class LobedBsdf:
    """A rough glass, uber, translucent or substrate entry: refpy_bsdf_full.FullBsdf.  `specular`: no lobe matches
    BSDF_ALL & ~BSDF_SPECULAR, so EstimateDirect's f is 0 (no shadow ray, no Tr draw) and its Sample_f has
    matchingComps == 0."""

    def __init__(self, b, uber):
        self.b, self.uber = b, uber
        self.none = b.none
        self.specular = not b.none and not b.matching(rf.BSDF_NON_SPECULAR)
        self.direct = _DirectView(b)

    def sample(self, q, wo, u0, u1, mode, stats=None, normals=None):
        s = self.b.sample(q, wo, u0, u1, rf.BSDF_ALL, mode, stats, normals)
        return None if s is None else s + (None,)


class Scene(rd.Scene):
    """refpy_distant.Scene whose table may hold entries of types 8 .. 11 (the classes below it see a matte in their
    place); self.lobed: the triangles under such an entry."""

    def __init__(self, s, lights=(), materials=(), triangle_material=(), *media_args, **kw):
        materials = list(materials)
        stand_in = []
        for m in materials:
            if m.type >= rf.ROUGH_GLASS:
                p = type(m)()
                p.type = rb.MATTE
                p.kd[0] = p.kd[1] = p.kd[2] = 0.5
                stand_in.append(p)
            else:
                stand_in.append(m)
        super().__init__(s, lights, stand_in, triangle_material, *media_args, **kw)
        table = {k: LobedBsdf(rf.FullBsdf.of(m), m.type == rf.UBER) for k, m in enumerate(materials)
                 if m.type >= rf.ROUGH_GLASS}
        self.lobed = set()
        for i, k in enumerate(triangle_material if materials else ()):
            if k in table:
                self.bsdf[i] = table[k]
                self.lobed.add(i)


def _tag(bsdf, typ):
    return typ | (1 << 8 if getattr(bsdf, "uber", False) else 0)


TAG_UBER = 1 << 8


# ---------------- photon pass ----------------
def walk(sc, rng, out, tags, o, d, depth, beta, med, max_depth, radius, tag, stats=None):
    """TracePhotonBeamRecursive, photonbeam.cpp:258-325, as refpy_passes_bsdf.walk; tags[k]: what spawned the ray
    of beam k."""
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
            walk(sc, rng, out, tags, add(o, mul(d, t)), wi, depth + 1, mul3(beta, trv), med, max_depth, radius, 0, stats)
        bm = med_tr(M, rng, o, d, tmax)
        if M is None:
            _count(stats, "vacuum_segment")
        out.append((o, hit[0], f32(radius), mul3(bm, beta)))
        tags.append(tag)
        tri = hit[2]
        q = sc.tris[tri]
        if sc.iface[tri]:  # :300-304
            _count(stats, "photon_pass")
            o = offset_origin(hit[0], hit[1], q["n"], d)
            med = sc.towards(tri, d, med)
            tag = 0
            continue
        bsdf = sc.bsdf[tri]
        ux, uy = rng.get2d()  # :313
        wo = tuple(-x for x in d)
        if bsdf.none:
            return
        s = bsdf.sample(q, wo, ux, uy, rs.IMPORTANCE, stats, sc.normals)
        if s is None:
            return
        wi, pdf, fr, typ, _ = s
        if pdf == 0 or all(x == 0 for x in fr):
            return
        n = q["n"]
        adw = f32(abs(dot(wi, n)))
        with np.errstate(all="ignore"):
            bn = tuple(f32(f32(f32(f32(bm[c] * beta[c]) * fr[c]) * adw) / pdf) for c in range(3))
        o = offset_origin(hit[0], hit[1], n, wi)  # isect.SpawnRay(wi): the far side after a transmission
        d = wi
        new_med = sc.towards(tri, wi, med)
        ratio = f32(f32(1) - f32(lum(bn) / lum(beta)))
        qrr = ratio if f32(0) < ratio else f32(0)
        if rng.uniform() < qrr:
            return
        med = new_med
        beta = tuple(f32(x / f32(f32(1) - qrr)) for x in bn)
        depth += 1
        tag = _tag(bsdf, typ) if tri in sc.lobed else 0
        if tag & rf.BSDF_TRANSMISSION:
            _count(stats, "photon_transmitted")
        if tag & TAG_UBER and tag & rf.BSDF_SPECULAR:
            _count(stats, "photon_uber_specular")


def trace_photon(sc, seq, max_depth, radius, tags, stats=None):
    """Beams of one photon (photonbeam.cpp:393-418), as refpy_distant.trace_photon."""
    rng = RNG(seq)
    out = []
    ln, light_pdf = sc.sample_light(rng.uniform())
    u0 = rng.get2d()
    u1 = rng.get2d()
    rng.uniform()  # uLightTime
    kind, idx = sc.all_lights[ln]
    if kind == "tri":
        L = sc.tris[idx]
        p, perr, nl, pdf_pos = sample_tri(L, *u0)
        if idx in sc.two_sided:
            wl, pdf_dir = rd.two_sided_direction(u1)
        else:
            wl = cosine_hemisphere(*u1)
            pdf_dir = f32(wl[2] * INV_PI)
        v1, v2 = coordinate_system(nl)
        w = add(add(mul(v1, wl[0]), mul(v2, wl[1])), mul(nl, wl[2]))
        o = offset_origin(p, perr, nl, w)
        Le = rd.area_L(sc, idx, nl, w)
        inside, outside = sc.pair[idx]
        med = outside if dot(w, nl) > 0 else inside
    else:
        D = sc.delta[idx]
        if D.kind == rd.LIGHT_DISTANT:
            o, w, Le, pdf_pos, pdf_dir = D.sample_le(u0)
            nl = w
            med = -1
        else:
            w, Le, pdf_dir = D.sample_le(u0)
            o, nl, pdf_pos = D.p, w, f32(1)
            med = sc.light_med[idx]
    if pdf_pos == 0 or pdf_dir == 0 or all(x == 0 for x in Le):
        return out
    ad = f32(abs(dot(nl, w)))
    den = f32(f32(light_pdf * pdf_pos) * pdf_dir)
    beta = tuple(f32(f32(ad * x) / den) for x in Le)
    if all(x == 0 for x in beta):
        return out
    walk(sc, rng, out, tags, o, w, 0, beta, med, max_depth, radius, 0, stats)
    return out


def trace_photons(sc, n_photons, iteration=0, max_depth=5, radius=0.01, first=None, stats=None):
    """Photons [0, first or n_photons) of a pass of n_photons: (the beams in order with per-photon counts, and per
    beam the tag of what spawned its ray: BxDFType bits, TAG_UBER on an uber surface)."""
    beams, counts, tags = [], [], []
    for i in range(first if first is not None else n_photons):
        b = trace_photon(sc, iteration * n_photons + i + 1, max_depth, radius, tags, stats)
        counts.append(len(b))
        beams.extend(b)
    return pack_beams(beams, counts), np.array(tags, np.int32)


# ---------------- camera pass ----------------
def camera_pass(sc, width, height, iteration=0, max_depth=5, render_surfaces=True, render_media=True, stats=None):
    """The camera paths of PhotonBeamIntegrator::Render (photonbeam.cpp:456-555), as refpy_distant.camera_pass:
    (segments + surface radiance, info) with info["lit_through"]: the pixels that gained radiance at a vertex
    reached through a transmitting bounce, and info["le_after_uber_specular"]: those that gained isect.Le after a
    specular bounce on an uber surface."""
    cam = rc.Camera(sc.struct, width, height)
    halton = rc.LazyHalton(width, height)
    emit = set(sc.lights)
    nl = len(sc.all_lights)
    segs = []
    surface = np.zeros((width * height, 3), np.float32)
    info = {"lit_through": set(), "le_after_uber_specular": set()}
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
            through = uber_specular = False
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
                    before = tuple(Ld)
                    if (depth == 0 or specular_bounce) and tri in emit:  # isect.Le(wo)
                        Le = rd.area_L(sc, tri, q["n"], wo)
                        Ld = [f32(Ld[c] + f32(beta[c] * Le[c])) for c in range(3)]
                        if depth > 0:
                            _count(stats, "le_after_specular")
                            if uber_specular and tuple(Ld) != before:
                                info["le_after_uber_specular"].add(pixel)
                    # UniformSampleOneLight (integrator.cpp:85-106): its three draws come whatever the material
                    ln = min(int(f32(smp.get1d() * f32(nl))), nl - 1)
                    light_pdf = f32(f32(1) / f32(nl))
                    ul = smp.get2d()
                    us = smp.get2d()
                    kind, idx = sc.all_lights[ln]
                    # EstimateDirect sees the BSDF under BSDF_ALL & ~BSDF_SPECULAR (integrator.cpp:112-113)
                    args = (sc, smp, hit[0], hit[1], q, getattr(bsdf, "direct", bsdf), tri, med, normalize(wo))
                    if bsdf.none:
                        ed = ZERO3
                    elif bsdf.specular:
                        ed = ZERO3  # f = 0: no shadow ray, no Tr draw; Sample_f has matchingComps == 0
                        _count(stats, "direct_no_matching_lobe" if tri in sc.lobed else "direct_early_out")
                    elif kind == "tri":
                        ed = rd.estimate_direct_area(*args, idx, us, ul, stats)
                    elif sc.delta[idx].kind == rd.LIGHT_DISTANT:
                        ed = rd.estimate_direct_distant(*args, sc.delta[idx], stats)
                    else:
                        ed = rpb.estimate_direct_delta(*args, sc.delta[idx], stats)
                    Ld = [f32(Ld[c] + f32(beta[c] * f32(ed[c] / light_pdf))) for c in range(3)]
                    if through and tuple(Ld) != before:
                        info["lit_through"].add(pixel)
                    if depth < max_depth - 1:
                        ux, uy = smp.get2d()
                        if bsdf.none:
                            break
                        s = bsdf.sample(q, wo, ux, uy, rs.RADIANCE, stats, sc.normals)
                        if s is None:
                            break
                        wi, pdf, f, typ, _ = s
                        if pdf == 0 or rc.black(f):
                            break
                        specular_bounce = (typ & rs.BSDF_SPECULAR) != 0  # :543, per sampled lobe
                        if tri in sc.lobed:
                            if typ & rf.BSDF_TRANSMISSION:
                                through = True
                                _count(stats, "camera_transmitted")
                            uber_specular = specular_bounce and bsdf.uber
                            if uber_specular:
                                _count(stats, "camera_uber_specular")
                        else:
                            uber_specular = False
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
    return pack_segments(segs, surface), info
