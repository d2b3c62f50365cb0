"""Pure-Python float32 restatement of the photon and camera passes with mirror and glass (test infrastructure).

Built on refpy_lights (scene, lights, emission) and refpy_camera (camera, sampler, EstimateDirect).  New
here, each from the reference text:
* FrDielectric (src/core/reflection.cpp:47-68), Refract (reflection.h:96-108);
* SpecularReflection::Sample_f (reflection.cpp:136-143) and FresnelSpecular::Sample_f (:477-511) inside
  BSDF::Sample_f (:703-768) for a BSDF with that one lobe (MirrorMaterial, mirror.cpp:45-56; GlassMaterial
  with zero roughness and allowMultipleLobes, glass.cpp:45-65);
* the walk of TracePhotonBeamRecursive (photonbeam.cpp:258-325) and the camera path (:478-555) with the
  material chosen per triangle: TransportMode::Importance for photons, Radiance for the camera;
  specularBounce and the isect.Le term; EstimateDirect on a specular vertex (no shadow ray, no Tr draw).
With every triangle mapped to -1 both passes are refpy_lights.trace_photons / refpy_camera.camera_pass.

`stats`, a dict, counts the branches taken (COUNTERS).  Every float operation is done on numpy float32
scalars in the reference's order.
"""
from __future__ import annotations

import numpy as np

import refpy_camera as rc
import refpy_lights as rl
from refpy_photon import (INV_PI, RNG, add, coordinate_system, cosine_hemisphere, dot, f32, grid_sample, grid_tr,
                          hg_sample, length, logf, mul, offset_origin)

MIRROR, GLASS = 1, 2
BSDF_REFLECTION, BSDF_TRANSMISSION, BSDF_SPECULAR = 1, 2, 16
IMPORTANCE, RADIANCE = 0, 1
COUNTERS = ("mirror_reflect", "glass_reflect", "transmit_enter", "transmit_leave", "tir", "refract_fail",
            "le_after_specular", "direct_early_out")
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


class Scene(rl.Scene):
    """refpy_lights.Scene plus self.mat: per triangle None (its matte kd) or a Mat."""

    def __init__(self, s, lights=(), materials=(), triangle_material=()):
        super().__init__(s, lights)
        table = [Mat.of(m) for m in materials]
        tm = list(triangle_material) if table else [-1] * len(self.tris)
        assert len(tm) == len(self.tris)
        self.mat = [None if k < 0 else table[k] for k in tm]


def _count(stats, key):
    if stats is not None and key in COUNTERS:
        stats[key] = stats.get(key, 0) + 1


def new_stats():
    return {k: 0 for k in COUNTERS}


# ---------------- photon pass ----------------
def walk(sc, rng, out, o, d, depth, beta, max_depth, radius, stats=None):
    """TracePhotonBeamRecursive, photonbeam.cpp:258-325, with the material's BSDF at :296-323."""
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
                 max_depth, radius, stats)
        if sc.medium and sc.grid:
            bm = (grid_tr(sc, rng, o, d, tmax),) * 3
        else:
            bm = sc.tr(d, tmax) if sc.medium else (f32(1),) * 3
        out.append((o, hit[0], f32(radius), tuple(f32(a * b) for a, b in zip(bm, beta))))
        q = sc.tris[hit[2]]
        m = sc.mat[hit[2]]
        ux, uy = rng.get2d()  # drawn before anything is known about the material (:313)
        wo = tuple(-x for x in d)
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
            wil, pdf, fr, _, branch = specular_sample(m, rc.to_local(q, wo), ux, IMPORTANCE)
            _count(stats, branch)
        if pdf == 0 or all(x == 0 for x in fr):
            return
        n = q["n"]
        wi = to_world(q, wil)
        adw = f32(abs(dot(wi, n)))
        bn = tuple(f32(f32(f32(f32(bm[c] * beta[c]) * fr[c]) * adw) / pdf) for c in range(3))
        o = offset_origin(hit[0], hit[1], n, wi)
        d = wi
        ratio = f32(f32(1) - f32(rl.lum(bn) / rl.lum(beta)))
        qrr = ratio if f32(0) < ratio else f32(0)
        if rng.uniform() < qrr:
            return
        beta = tuple(f32(x / f32(f32(1) - qrr)) for x in bn)
        depth += 1


def trace_photon(sc, seq, max_depth, radius, stats=None):
    """Beams of one photon (photonbeam.cpp:393-418): refpy_lights.trace_photon's emission, this walk."""
    rng = RNG(seq)
    out = []
    ln, light_pdf = sc.sample_light(rng.uniform())
    u0 = rng.get2d()
    u1 = rng.get2d()
    rng.uniform()  # uLightTime
    kind, idx = sc.all_lights[ln]
    if kind == "tri":
        L = sc.tris[idx]
        p, perr, nl, pdf_pos = sc.sample_tri(L, *u0)
        wl = cosine_hemisphere(*u1)
        pdf_dir = f32(wl[2] * INV_PI)
        v1, v2 = coordinate_system(nl)
        w = add(add(mul(v1, wl[0]), mul(v2, wl[1])), mul(nl, wl[2]))
        o = offset_origin(p, perr, nl, w)
        Le = L["Le"] if dot(nl, w) > 0 else ZERO3
    else:
        D = sc.delta[idx]
        w, Le, pdf_dir = D.sample_le(u0)
        o, nl, pdf_pos = D.p, w, f32(1)
    if pdf_pos == 0 or pdf_dir == 0 or all(x == 0 for x in Le):
        return out
    ad = f32(abs(dot(nl, w)))
    den = f32(f32(light_pdf * pdf_pos) * pdf_dir)
    beta = tuple(f32(f32(ad * x) / den) for x in Le)
    if all(x == 0 for x in beta):
        return out
    walk(sc, rng, out, o, w, 0, beta, max_depth, radius, stats)
    return out


def trace_photons(scene_struct, lights, materials, triangle_material, n_photons, iteration=0, max_depth=5,
                  radius=0.01, stats=None):
    """The whole pass (sequences iteration*N + i + 1), as refpy_lights.trace_photons returns it."""
    sc = Scene(scene_struct, lights, materials, triangle_material)
    beams, counts = [], []
    for i in range(n_photons):
        b = trace_photon(sc, iteration * n_photons + i + 1, max_depth, radius, stats)
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


# ---------------- camera pass ----------------
def camera_pass(scene_struct, lights, materials, triangle_material, width, height, iteration=0, max_depth=5,
                render_surfaces=True, render_media=True, stats=None):
    """refpy_camera.camera_pass with the material's BSDF at the vertex (photonbeam.cpp:512-554)."""
    sc = Scene(scene_struct, lights, materials, triangle_material)
    cam = rc.Camera(scene_struct, width, height)
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
            beta = (f32(1),) * 3
            Ld = [f32(0)] * 3
            pixel = py * width + px
            specular_bounce = False
            for depth in range(max_depth):
                hit, tmax = rc.intersect(sc, o, d)
                if hit is None:
                    break
                mb = rc.medium_tr(sc, smp, o, d, tmax) if sc.medium else (f32(1),) * 3
                if render_media:
                    segs.append((o, hit[0], d, tmax, pixel, depth))
                beta = tuple(f32(b * m) for b, m in zip(beta, mb))
                if not render_surfaces:
                    break
                q = sc.tris[hit[2]]
                m = sc.mat[hit[2]]
                if m is not None and m.none:  # a BSDF without a BxDF: as a black kd
                    q = dict(q, kd=ZERO3)
                    m = None
                wo = rc.neg(d)
                if (depth == 0 or specular_bounce) and hit[2] in emit and dot(q["n"], wo) > 0:  # isect.Le(wo)
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
                    ed = rc.estimate_direct_area(sc, smp, hit[0], hit[1], q, rc.normalize(wo), idx, us, ul, None)
                else:
                    ed = rc.estimate_direct_delta(sc, smp, hit[0], hit[1], q, rc.normalize(wo), sc.delta[idx], None)
                Ld = [f32(Ld[c] + f32(beta[c] * f32(ed[c] / light_pdf))) for c in range(3)]
                if depth < max_depth - 1:
                    ux, uy = smp.get2d()
                    if m is None:
                        bs = rc.bsdf_sample(q, wo, ux, uy)
                        if bs is None or rc.black(bs[2]):
                            break
                        wi, pdf, f = bs
                        specular_bounce = False
                    else:
                        wil, pdf, f, typ, branch = specular_sample(m, rc.to_local(q, wo), ux, RADIANCE)
                        _count(stats, branch)
                        if pdf == 0 or rc.black(f):
                            break
                        wi = to_world(q, wil)
                        specular_bounce = (typ & BSDF_SPECULAR) != 0
                    ad = f32(abs(dot(wi, q["n"])))
                    beta = tuple(f32(beta[c] * f32(f32(f[c] * ad) / pdf)) for c in range(3))
                    o = offset_origin(hit[0], hit[1], q["n"], wi)
                    d = wi
                y = rl.lum(beta)
                if y < f32(0.25):
                    cp = f32(1) if f32(1) < y else y
                    if smp.get1d() > cp:
                        break
                    beta = tuple(f32(b / cp) for b in beta)
            if render_surfaces:
                surface[pixel] += np.array(Ld, np.float32)
    n = len(segs)
    out = {"o": np.zeros((n, 3), np.float32), "p": np.zeros((n, 3), np.float32), "d": np.zeros((n, 3), np.float32),
           "tmax": np.zeros(n, np.float32), "pixel": np.zeros(n, np.int32), "depth": np.zeros(n, np.int32)}
    for k, (o, p, d, t, pix, dep) in enumerate(segs):
        out["o"][k], out["p"][k], out["d"][k], out["tmax"][k], out["pixel"][k], out["depth"][k] = o, p, d, t, pix, dep
    out["surface"] = surface
    return out
