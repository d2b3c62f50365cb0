"""The camera, its sampler and the matte BSDF of the pure-Python float32 restatement (test infrastructure),
from the reference text: AwesomeSampler over HaltonSampler with its 1000-dimension switch
(src/integrators/photonbeam.cpp:188-224, 456-462), the pinhole ray of PerspectiveCamera
(src/cameras/perspective.cpp), the Lambertian BSDF (src/core/reflection.cpp:650-768) and PowerHeuristic.
The camera pass that uses them is tests/refpy_passes.py.
"""
from __future__ import annotations

import ctypes

import refpy_photon as rp
from refpy_photon import INV_PI, PI, RNG, add, cosine_hemisphere, cross, dot, f32, gamma, mul, normalize, sub, vabs

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
