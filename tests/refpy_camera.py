"""Pure-Python float32 restatement of the camera pass (test infrastructure).

The camera path of PhotonBeamIntegrator::Render (src/integrators/photonbeam.cpp:456-555) written from
the reference text: AwesomeSampler over HaltonSampler with its 1000-dimension switch (:188-224, 456-462),
the pinhole ray of PerspectiveCamera (src/cameras/perspective.cpp), Scene::Intersect, both media,
UniformSampleOneLight / EstimateDirect (src/core/integrator.cpp:85-214) for diffuse area lights (with
MIS) and for delta lights (PointLight / SpotLight: Sample_Li of point.cpp:44-53 and spot.cpp:53-62, the
shadow ray of VisibilityTester::Tr, no MIS), the Lambertian bounce and the roulette.  Built on
refpy_photon (vectors, RNG, Halton, media) and refpy_lights (the merged light list, Falloff).  Pinned bit
for bit to oracle.camera_pass on area-light scenes by tests/test_lights_refpy.py.
"""
from __future__ import annotations

import ctypes

import numpy as np

import refpy_lights as rl
import refpy_photon as rp
from refpy_photon import (INF, INV_PI, ONE_MINUS_EPS, PI, RNG, add, cosine_hemisphere, cross, dot, f32, gamma, length,
                          mul, normalize, offset_origin, sub, vabs)

rp._libm.tanf.argtypes = [ctypes.c_float]
rp._libm.tanf.restype = ctypes.c_float
HALTON_DIMS = 1000  # HaltonSampler's PrimeTableSize = AwesomeSampler's limit (photonbeam.cpp:460)


def lensq(v):
    return dot(v, v)


def neg(v):
    return tuple(-x for x in v)


def black(s):
    return all(x == 0 for x in s)


class LazyHalton(rp.Halton):
    """refpy_photon.Halton whose prime table and permutations (drawn from one RNG in prime order) grow
    on demand: a camera path rarely reaches dimension 100 of the 1000."""

    def __init__(self, width, height):
        super().__init__(width, height, ndims=0)
        self._rng = rp.DefaultRNG()
        self._next = 2

    def sample(self, index, dim):
        while len(self.primes) <= dim:
            c = self._next
            while not all(c % q for q in self.primes if q * q <= c):
                c += 1
            self._next = c + 1
            self.primes.append(c)
            self.perms.append(rp.shuffle(list(range(c)), self._rng))
        return super().sample(index, dim)


class AwesomeSampler:
    """AwesomeSampler(0, tileSampler, 1000, GoodPixelIndex), photonbeam.cpp:188-224."""

    def __init__(self, halton, index, seq):
        self.h, self.index, self.count, self.rng = halton, index, 0, RNG(seq)

    def get1d(self):
        self.count += 1
        if self.count <= HALTON_DIMS:
            return self.h.sample(self.index, self.count - 1)
        return self.rng.uniform()

    uniform = get1d  # the media of refpy_photon draw through .uniform()

    def get2d(self):
        self.count += 2
        if self.count <= HALTON_DIMS:
            return self.h.sample(self.index, self.count - 2), self.h.sample(self.index, self.count - 1)
        return self.rng.get2d()


def good_pixel_index(W, H, px, py):
    """iterNumPixels in the single-threaded order: 16x16 tiles row-major, x fastest inside (:345-347, 456-458)."""
    tx, ty = px >> 4, py >> 4
    th, tw = min(16, H - ty * 16), min(16, W - tx * 16)
    return ty * 16 * W + tx * 16 * th + (py & 15) * tw + (px & 15)


class Camera:
    """LookAt frame and screen window of the perspective camera (perspective.cpp, transform.cpp LookAt)."""

    def __init__(self, s, width, height):
        self.pos = tuple(f32(x) for x in s.cam_pos)
        look = tuple(f32(x) for x in s.cam_look)
        up = tuple(f32(x) for x in s.cam_up)
        self.dir = normalize(sub(look, self.pos))
        self.right = normalize(cross(normalize(up), self.dir))
        self.nup = cross(self.dir, self.right)
        aspect = f32(f32(width) / f32(height))
        if aspect > 1:
            self.win = (-aspect, aspect, f32(-1), f32(1))
        else:
            self.win = (f32(-1), f32(1), f32(f32(-1) / aspect), f32(f32(1) / aspect))
        self.tan = f32(rp._libm.tanf(float(f32(f32(f32(PI / f32(180)) * f32(s.cam_fov_deg)) / f32(2)))))
        self.fw, self.fh = f32(width), f32(height)

    def ray(self, fx, fy):
        sx0, sx1, sy0, sy1 = self.win
        sx = f32(sx0 + f32(f32(fx / self.fw) * f32(sx1 - sx0)))
        sy = f32(sy1 - f32(f32(fy / self.fh) * f32(sy1 - sy0)))
        dc = normalize((f32(sx * self.tan), f32(sy * self.tan), f32(1)))
        d = add(add(mul(self.right, dc[0]), mul(self.nup, dc[1])), mul(self.dir, dc[2]))
        o = self.pos
        oerr = mul(vabs(self.pos), gamma(3))  # Transform::operator()(Ray): the origin's error bound
        l2 = lensq(d)
        if l2 > 0:
            o = add(o, mul(d, f32(dot(vabs(d), oerr) / l2)))
        return o, d


def intersect(sc, o, d, tmax=INF):
    """Scene::Intersect against ray.tMax: ((p, pError, triangle) or None, tMax)."""
    best = None
    for i, T in enumerate(sc.tris):
        h = sc.hit_tri(T, o, d, tmax)
        if h is None:
            continue
        tmax = h[0]
        best = (h[1], h[2], i)
    return best, tmax


def medium_tr(sc, smp, o, d, tmax):
    if sc.grid:
        return (rp.grid_tr(sc, smp, o, d, tmax),) * 3
    return sc.tr(d, tmax)


# ---- matte BSDF (reflection.cpp:650-768) ----
def to_local(q, v):
    return (dot(v, q["ss"]), dot(v, q["ts"]), dot(v, q["n"]))


def absorbing(q):
    return all(x == 0 for x in q["kd"])


def bsdf_f(q, wo, wi):
    if absorbing(q) or to_local(q, wo)[2] == 0:
        return (f32(0),) * 3
    if f32(dot(wi, q["n"]) * dot(wo, q["n"])) > 0:
        return tuple(f32(f32(0) + f32(k * INV_PI)) for k in q["kd"])
    return (f32(0),) * 3


def bsdf_pdf(q, wo, wi):
    if absorbing(q):
        return f32(0)
    lo, li = to_local(q, wo), to_local(q, wi)
    if lo[2] == 0:
        return f32(0)
    return f32(abs(li[2]) * INV_PI) if f32(lo[2] * li[2]) > 0 else f32(0)


def bsdf_sample(q, wo, ux, uy):
    """BSDF::Sample_f: (wi, pdf, f) or None where f = 0."""
    if absorbing(q):
        return None
    lo = to_local(q, wo)
    if lo[2] == 0:
        return None
    wl = list(cosine_hemisphere(ux, uy))
    if lo[2] < 0:
        wl[2] = f32(wl[2] * f32(-1))
    pdf = f32(abs(wl[2]) * INV_PI) if f32(lo[2] * wl[2]) > 0 else f32(0)
    if pdf == 0:
        return None
    ss, ts, n = q["ss"], q["ts"], q["n"]
    wi = tuple(f32(f32(f32(ss[i] * wl[0]) + f32(ts[i] * wl[1])) + f32(n[i] * wl[2])) for i in range(3))
    return wi, pdf, tuple(f32(k * INV_PI) for k in q["kd"])


def power_heuristic(fp, gp):
    f, g = f32(f32(1) * fp), f32(f32(1) * gp)
    return f32(f32(f * f) / f32(f32(f * f) + f32(g * g)))


def shadow_ray(sc, smp, p, perr, q, target_p, target_err, target_n, Li, stats):
    """VisibilityTester::Tr (light.cpp:63-81) over SpawnRayTo (interaction.h:73-78): Li after it."""
    ro = offset_origin(p, perr, q["n"], sub(target_p, p))
    target = offset_origin(target_p, target_err, target_n, sub(ro, target_p))
    rd = sub(target, ro)
    tmax = f32(f32(1) - f32(0.0001))
    hit, _ = intersect(sc, ro, rd, tmax)
    if stats is not None:
        stats["shadow_blocked" if hit is not None else "shadow_clear"] += 1
    if hit is not None:
        return (f32(0),) * 3  # every triangle has a material
    if sc.medium:
        tr = medium_tr(sc, smp, ro, rd, tmax)
        return tuple(f32(a * f32(f32(1) * b)) for a, b in zip(Li, tr))
    return Li


def estimate_direct_delta(sc, smp, p, perr, q, wo, D, stats):
    """EstimateDirect with IsDeltaLight (integrator.cpp:108-165): no MIS weight, no BSDF-sampling half."""
    wi = normalize(sub(D.p, p))  # Sample_Li: point.cpp:44-53, spot.cpp:53-62
    fo = D.falloff(neg(wi))
    dist2 = lensq(sub(D.p, p))
    Li = tuple(f32(f32(c * fo) / dist2) for c in D.I)
    zero = (f32(0),) * 3
    if black(Li):
        return zero
    ad = f32(abs(dot(wi, q["n"])))
    f = tuple(f32(x * ad) for x in bsdf_f(q, wo, wi))
    if black(f):
        return zero
    Li = shadow_ray(sc, smp, p, perr, q, D.p, zero, zero, Li, stats)
    if black(Li):
        return zero
    return tuple(f32(f32(0) + f32(f32(a * b) / f32(1))) for a, b in zip(f, Li))


def estimate_direct_area(sc, smp, p, perr, q, wo, li, us, ul, stats):
    """EstimateDirect for the DiffuseAreaLight on triangle li, handleMedia = true (integrator.cpp:108-214)."""
    L = sc.tris[li]
    Ld = [f32(0)] * 3
    sp, sperr, sn, light_pdf = sc.sample_tri(L, *ul)  # Shape::Sample(ref, u), shape.cpp:56-70
    w = sub(sp, p)
    if lensq(w) == 0:
        light_pdf = f32(0)
    else:
        w = normalize(w)
        with np.errstate(divide="ignore"):
            light_pdf = f32(light_pdf * f32(lensq(sub(p, sp)) / f32(abs(dot(sn, neg(w))))))
        if np.isinf(light_pdf):
            light_pdf = f32(0)
    Li = (f32(0),) * 3
    if light_pdf == 0 or lensq(sub(sp, p)) == 0:
        light_pdf = f32(0)
    else:
        wi = normalize(sub(sp, p))
        if dot(sn, neg(wi)) > 0:  # DiffuseAreaLight::L, one-sided
            Li = L["Le"]
    if light_pdf > 0 and not black(Li):
        ad = f32(abs(dot(wi, q["n"])))
        f = tuple(f32(x * ad) for x in bsdf_f(q, wo, wi))
        scat_pdf = bsdf_pdf(q, wo, wi)
        if not black(f):
            Li = shadow_ray(sc, smp, p, perr, q, sp, sperr, sn, Li, stats)
            if not black(Li):
                wgt = power_heuristic(light_pdf, scat_pdf)
                Ld = [f32(Ld[c] + f32(f32(f32(f[c] * Li[c]) * wgt) / light_pdf)) for c in range(3)]
    bs = bsdf_sample(q, wo, *us)
    if bs is None:
        return tuple(Ld)
    wi, scat_pdf, f = bs
    ad = f32(abs(dot(wi, q["n"])))
    f = tuple(f32(x * ad) for x in f)
    if black(f) or not scat_pdf > 0:
        return tuple(Ld)
    ro = offset_origin(p, perr, q["n"], wi)
    hl = sc.hit_tri(L, ro, wi, INF)  # Shape::Pdf(ref, wi), shape.cpp:72-87: this triangle alone
    if hl is None:
        return tuple(Ld)
    with np.errstate(divide="ignore"):
        light_pdf = f32(lensq(sub(p, hl[1])) / f32(f32(abs(dot(L["n"], neg(wi)))) * L["area"]))
    if np.isinf(light_pdf) or light_pdf == 0:
        return tuple(Ld)
    wgt = power_heuristic(scat_pdf, light_pdf)
    found, tmax = intersect(sc, ro, wi)
    tr = (f32(1),) * 3
    if sc.medium:
        tr = tuple(f32(a * b) for a, b in zip(tr, medium_tr(sc, smp, ro, wi, tmax)))
    if found is not None and found[2] == li and dot(L["n"], neg(wi)) > 0 and not black(L["Le"]):
        Ld = [f32(Ld[c] + f32(f32(f32(f32(f[c] * L["Le"][c]) * tr[c]) * wgt) / scat_pdf)) for c in range(3)]
    return tuple(Ld)


def camera_pass(scene_struct, lights, width, height, iteration=0, max_depth=5, render_surfaces=True,
                render_media=True, stats=None):
    """Segments in row-major pixel order (depth order within a pixel) + surface radiance (W*H, 3), as
    oracle.camera_pass returns them.  `stats`, a dict, counts blocked and clear shadow rays."""
    sc = rl.Scene(scene_struct, lights)
    if stats is not None:
        stats.setdefault("shadow_blocked", 0)
        stats.setdefault("shadow_clear", 0)
    cam = Camera(scene_struct, width, height)
    halton = LazyHalton(width, height)
    emit = set(sc.lights)
    nl = len(sc.all_lights)
    segs = []
    surface = np.zeros((width * height, 3), np.float32)
    for py in range(height):
        for px in range(width):
            smp = AwesomeSampler(halton, halton.index(px, py, iteration), good_pixel_index(width, height, px, py))
            fx, fy = smp.get2d()
            smp.get1d()  # time
            smp.get2d()  # lens (pinhole)
            o, d = cam.ray(f32(f32(px) + fx), f32(f32(py) + fy))
            beta = (f32(1),) * 3
            Ld = [f32(0)] * 3
            pixel = py * width + px
            for depth in range(max_depth):
                hit, tmax = intersect(sc, o, d)
                if hit is None:
                    break  # area and delta lights: Le(ray) = 0
                mb = medium_tr(sc, smp, o, d, tmax) if sc.medium else (f32(1),) * 3
                if render_media:
                    segs.append((o, hit[0], d, tmax, pixel, depth))
                beta = tuple(f32(b * m) for b, m in zip(beta, mb))
                if not render_surfaces:
                    break
                q = sc.tris[hit[2]]
                wo = neg(d)
                if depth == 0 and hit[2] in emit and dot(q["n"], wo) > 0:  # isect.Le(wo)
                    Ld = [f32(Ld[c] + f32(beta[c] * q["Le"][c])) for c in range(3)]
                # UniformSampleOneLight (integrator.cpp:85-106)
                ln = min(int(f32(smp.get1d() * f32(nl))), nl - 1)
                light_pdf = f32(f32(1) / f32(nl))
                ul = smp.get2d()
                us = smp.get2d()
                kind, idx = sc.all_lights[ln]
                if kind == "tri":
                    ed = estimate_direct_area(sc, smp, hit[0], hit[1], q, normalize(wo), idx, us, ul, stats)
                else:
                    ed = estimate_direct_delta(sc, smp, hit[0], hit[1], q, normalize(wo), sc.delta[idx], stats)
                Ld = [f32(Ld[c] + f32(beta[c] * f32(ed[c] / light_pdf))) for c in range(3)]
                if depth < max_depth - 1:
                    bs = bsdf_sample(q, wo, *smp.get2d())
                    if bs is None or black(bs[2]):
                        break
                    wi, pdf, f = bs
                    ad = f32(abs(dot(wi, q["n"])))
                    beta = tuple(f32(beta[c] * f32(f32(f[c] * ad) / pdf)) for c in range(3))
                    o = offset_origin(hit[0], hit[1], q["n"], wi)
                    d = wi
                y = rl.lum(beta)
                if y < f32(0.25):
                    cp = f32(1) if f32(1) < y else y  # std::min((Float)1, beta.y())
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
