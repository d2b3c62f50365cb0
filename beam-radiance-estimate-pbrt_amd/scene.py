"""ctypes mirror of include/bre_scene.h and the benchmark scene of SURVEY.md §8d (C1/C2).

Pure data: the same struct the C ABI takes (``bre_trace_photons``) and the oracle restatement
reads (``ora_trace_photons``).  ``cornell_scene`` must stay identical to libbre's
``bre_scene_cornell`` (checked byte for byte by tests/test_photon_oracle.py).
"""
from __future__ import annotations

import ctypes

MAX_TRIANGLES = 128               # inline in Scene.triangles
MAX_SCENE_TRIANGLES = 1 << 24     # through Scene.triangles_ext
MAX_DEPTH = 16
MEDIUM_NONE, MEDIUM_HOMOGENEOUS, MEDIUM_GRID = 0, 1, 2

F3 = ctypes.c_float * 3


class Triangle(ctypes.Structure):
    """bre_triangle: one pbrt Triangle (world-space vertices in mesh index order)."""
    _fields_ = [("p", F3 * 3), ("kd", F3), ("Le", F3), ("emit", ctypes.c_int32), ("flip", ctypes.c_int32)]


class Scene(ctypes.Structure):
    _fields_ = [("n_triangles", ctypes.c_int32),
                ("has_medium", ctypes.c_int32), ("sigma_a", F3), ("sigma_s", F3), ("g", ctypes.c_float),
                ("cam_pos", F3), ("cam_look", F3), ("cam_up", F3), ("cam_fov_deg", ctypes.c_float),
                ("triangles", Triangle * MAX_TRIANGLES),
                ("grid_n", ctypes.c_int32 * 3), ("world_to_medium", ctypes.c_float * 16),
                ("grid_density", ctypes.c_void_p), ("triangles_ext", ctypes.c_void_p)]

    def to_bytes(self) -> bytes:
        return ctypes.string_at(ctypes.addressof(self), ctypes.sizeof(self))


LIGHT_POINT, LIGHT_SPOT = 1, 2
MAX_LIGHTS = 1024


class Light(ctypes.Structure):
    """bre_light: a PointLight or SpotLight (row-major 4x4 transforms, `order` = triangles declared before it)."""
    _fields_ = [("type", ctypes.c_int32), ("I", F3), ("light_to_world", ctypes.c_float * 16),
                ("world_to_light", ctypes.c_float * 16), ("cone_total_deg", ctypes.c_float),
                ("cone_falloff_start_deg", ctypes.c_float), ("order", ctypes.c_int32)]

    def to_bytes(self) -> bytes:
        return ctypes.string_at(ctypes.addressof(self), ctypes.sizeof(self))


def point_light(p, I, order: int = 0) -> Light:
    """LightSource "point" at `p` under an identity CTM: LightToWorld = Translate(p) (point.cpp:80-88)."""
    L = Light()
    L.type = LIGHT_POINT
    L.I = _f3(I)
    for i in range(4):
        L.light_to_world[5 * i] = L.world_to_light[5 * i] = 1.0
    for k in range(3):
        L.light_to_world[4 * k + 3] = float(p[k])
        L.world_to_light[4 * k + 3] = -float(p[k])
    L.order = int(order)
    return L


def spot_light(frm, to, I, coneangle: float = 30.0, conedelta: float = 5.0, order: int = 0, ctm=None,
               ctm_inv=None) -> Light:
    """LightSource "spot" (spot.cpp:104-124), built by the host library's parser code
    (bre_pbrt_make_spot_light) so that the matrices are the reference's."""
    from .pbrt import make_spot_light

    return make_spot_light(frm, to, I, coneangle, conedelta, order, ctm, ctm_inv)


LIGHT_DISTANT = 3
EMIT_ONE_SIDED, EMIT_TWO_SIDED = 1, 2  # bre_triangle.emit


class two_sided(tuple):
    """The Le of a mesh tuple, marked as a two-sided emitter: make_scene sets emit = EMIT_TWO_SIDED."""


def distant_light(frm, to, L, order: int = 0, light_to_world=None) -> Light:
    """LightSource "distant" (distant.cpp:43-47, 94-102): I = L and, in light_to_world[0..2], the world-space
    wLight = Normalize(LightToWorld(from - to)), computed in float32 with Transform::operator()(Vector3f)'s and
    Normalize's own operations.  `light_to_world`: the CTM as 16 row-major floats or a 4x4 (None: identity).
    Every other field of the record stays 0 (bre_scene.h)."""
    import numpy as np

    f = np.float32
    m = np.eye(4, dtype=f) if light_to_world is None else np.asarray(light_to_world, f).reshape(4, 4)
    d = [f(f(frm[k]) - f(to[k])) for k in range(3)]  # Point3f - Point3f
    # transform.h:236-242: m[i][0] * x + m[i][1] * y + m[i][2] * z
    w = [f(f(f(m[i][0] * d[0]) + f(m[i][1] * d[1])) + f(m[i][2] * d[2])) for i in range(3)]
    # Normalize: v / Length(v); Vector3::operator/ multiplies by the reciprocal (geometry.h)
    length = f(np.sqrt(f(f(f(w[0] * w[0]) + f(w[1] * w[1])) + f(w[2] * w[2]))))
    with np.errstate(all="ignore"):
        inv = f(f(1) / length)
    out = Light()
    out.type = LIGHT_DISTANT
    out.I = _f3(L)
    for k in range(3):
        out.light_to_world[k] = float(f(w[k] * inv))
    out.order = int(order)
    return out


MATERIAL_MIRROR, MATERIAL_GLASS = 1, 2
MAX_MATERIALS = 1024


class Material(ctypes.Structure):
    """bre_material: a MirrorMaterial or a GlassMaterial with zero roughness (32 bytes)."""
    _fields_ = [("type", ctypes.c_int32), ("kr", F3), ("kt", F3), ("eta", ctypes.c_float)]

    def to_bytes(self) -> bytes:
        return ctypes.string_at(ctypes.addressof(self), ctypes.sizeof(self))


def _rgb(v):
    return F3(*([float(v)] * 3 if isinstance(v, (int, float)) else [float(x) for x in v]))


def mirror(kr=0.9) -> Material:
    """Material "mirror" (mirror.cpp:58-64): "Kr" (rgb or scalar, default 0.9)."""
    return Material(MATERIAL_MIRROR, _rgb(kr), _rgb(0.0), 1.0)


def glass(kr=1.0, kt=1.0, eta: float = 1.5) -> Material:
    """Material "glass" with zero roughness (glass.cpp:94-109): "Kr", "Kt" (default 1), "eta" (1.5)."""
    return Material(MATERIAL_GLASS, _rgb(kr), _rgb(kt), float(eta))


MATERIAL_MATTE, MATERIAL_PLASTIC, MATERIAL_METAL = 4, 5, 6


class MaterialEx(ctypes.Structure):
    """bre_material_ex: the wide record (112 bytes), a Material followed by the parameters of pbrt's matte,
    plastic and metal."""
    _fields_ = [("type", ctypes.c_int32), ("kr", F3), ("kt", F3), ("eta", ctypes.c_float),
                ("kd", F3), ("ks", F3), ("ceta", F3), ("ck", F3), ("roughness", ctypes.c_float),
                ("uroughness", ctypes.c_float), ("vroughness", ctypes.c_float), ("sigma", ctypes.c_float),
                ("remap", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]

    def to_bytes(self) -> bytes:
        return ctypes.string_at(ctypes.addressof(self), ctypes.sizeof(self))

    @property
    def opacity(self):
        """An uber's "opacity": the words of `ceta`, which an uber never reads (the record's anonymous union)."""
        return self.ceta

    @opacity.setter
    def opacity(self, v):
        self.ceta = v

    @property
    def amount(self):
        """A mix's "amount": the words of `kd`, which a mix never reads (the record's anonymous union)."""
        return self.kd

    @amount.setter
    def amount(self, v):
        self.kd = v

    @property
    def mix_child(self):
        """A mix's two children, table indices: a view of reserved[0..1] (writable by index)."""
        return (ctypes.c_int32 * 2).from_address(ctypes.addressof(self) + type(self).reserved.offset)

    @mix_child.setter
    def mix_child(self, v):
        self.reserved[0], self.reserved[1] = int(v[0]), int(v[1])


def widen(m) -> "MaterialEx":
    """A Material as the MaterialEx bre_set_materials makes of it; a MaterialEx as it is."""
    if isinstance(m, MaterialEx):
        return m
    w = MaterialEx()
    ctypes.memmove(ctypes.addressof(w), ctypes.addressof(m), ctypes.sizeof(Material))
    return w


def matte(kd=0.5, sigma: float = 0.0) -> MaterialEx:
    """Material "matte" (matte.cpp:64-71): "Kd" (rgb or scalar, default 0.5), "sigma" in degrees (0: Lambertian,
    otherwise Oren-Nayar)."""
    m = MaterialEx()
    m.type, m.kd, m.sigma = MATERIAL_MATTE, _rgb(kd), float(sigma)
    return m


def plastic(kd=0.25, ks=0.25, roughness: float = 0.1, remap: bool = True) -> MaterialEx:
    """Material "plastic" (plastic.cpp:72-83): "Kd", "Ks" (default 0.25), "roughness" (0.1), "remaproughness"."""
    m = MaterialEx()
    m.type, m.kd, m.ks, m.roughness, m.remap = MATERIAL_PLASTIC, _rgb(kd), _rgb(ks), float(roughness), int(bool(remap))
    return m


def metal(eta, k, roughness: float = 0.01, uroughness: float = 0.0, vroughness: float = 0.0,
          remap: bool = True) -> MaterialEx:
    """Material "metal" (metal.cpp) with explicit "eta" and "k" (rgb or scalar): "roughness" (default 0.01),
    "uroughness" / "vroughness" (0: not given, `roughness` is used), "remaproughness"."""
    m = MaterialEx()
    m.type, m.ceta, m.ck = MATERIAL_METAL, _rgb(eta), _rgb(k)
    m.roughness, m.uroughness, m.vroughness, m.remap = float(roughness), float(uroughness), float(vroughness), int(bool(remap))
    return m


MATERIAL_ROUGH_GLASS, MATERIAL_UBER, MATERIAL_TRANSLUCENT, MATERIAL_SUBSTRATE = 8, 9, 10, 11


def rough_glass(kr=1.0, kt=1.0, eta: float = 1.5, uroughness: float = 0.0, vroughness: float = 0.0,
                remap: bool = True) -> MaterialEx:
    """Material "glass" with "uroughness" or "vroughness" != 0 (glass.cpp:94-110): "Kr", "Kt" (default 1), "eta"
    (1.5), the two roughnesses (default 0; both 0 is glass(), and refused as a rough glass), "remaproughness"."""
    m = MaterialEx()
    m.type, m.kr, m.kt, m.eta = MATERIAL_ROUGH_GLASS, _rgb(kr), _rgb(kt), float(eta)
    m.uroughness, m.vroughness, m.remap = float(uroughness), float(vroughness), int(bool(remap))
    return m


def uber(kd=0.25, ks=0.25, kr=0.0, kt=0.0, roughness: float = 0.1, uroughness: float = 0.0, vroughness: float = 0.0,
         eta: float = 1.5, opacity=1.0, remap: bool = True) -> MaterialEx:
    """Material "uber" (uber.cpp:103-127): "Kd", "Ks" (default 0.25), "Kr", "Kt" (0), "roughness" (0.1),
    "uroughness" / "vroughness" (0: not given; u falls back to `roughness`, v to u), "eta" (1.5), "opacity" (1),
    "remaproughness"."""
    m = MaterialEx()
    m.type, m.kd, m.ks, m.kr, m.kt = MATERIAL_UBER, _rgb(kd), _rgb(ks), _rgb(kr), _rgb(kt)
    m.roughness, m.uroughness, m.vroughness = float(roughness), float(uroughness), float(vroughness)
    m.eta, m.opacity, m.remap = float(eta), _rgb(opacity), int(bool(remap))
    return m


def translucent(kd=0.25, ks=0.25, reflect=0.5, transmit=0.5, roughness: float = 0.1, remap: bool = True) -> MaterialEx:
    """Material "translucent" (translucent.cpp:82-98): "Kd", "Ks" (default 0.25), "reflect", "transmit" (0.5; kept
    in kr and kt), "roughness" (0.1), "remaproughness"."""
    m = MaterialEx()
    m.type, m.kd, m.ks, m.kr, m.kt = MATERIAL_TRANSLUCENT, _rgb(kd), _rgb(ks), _rgb(reflect), _rgb(transmit)
    m.roughness, m.remap = float(roughness), int(bool(remap))
    return m


def substrate(kd=0.5, ks=0.5, uroughness: float = 0.1, vroughness: float = 0.1, remap: bool = True) -> MaterialEx:
    """Material "substrate" (substrate.cpp:67-81): "Kd", "Ks" (default 0.5), "uroughness", "vroughness" (0.1),
    "remaproughness"."""
    m = MaterialEx()
    m.type, m.kd, m.ks = MATERIAL_SUBSTRATE, _rgb(kd), _rgb(ks)
    m.uroughness, m.vroughness, m.remap = float(uroughness), float(vroughness), int(bool(remap))
    return m


MATERIAL_MIX = 12
MAX_MIX_DEPTH, MAX_BXDFS = 4, 8


def mix(child1: int, child2: int, amount=0.5) -> MaterialEx:
    """Material "mix" (mixmat.cpp:66-72): the table indices of "namedmaterial1" and "namedmaterial2", both earlier
    entries of the table the record goes into, and "amount" (rgb or scalar, default 0.5): the first child's BxDFs
    scaled by amount, then the second's by 1 - amount."""
    m = MaterialEx()
    m.type, m.amount, m.mix_child = MATERIAL_MIX, _rgb(amount), (int(child1), int(child2))
    return m


def scene_materials(meshes):
    """(materials, triangle_material) of `meshes` for BeamGather.set_materials: one table entry per
    distinct Material / MaterialEx object, in order of first use, and per triangle its index (-1: the mesh has
    no fifth element, or None there).  With a MaterialEx among them the whole table is returned wide."""
    table, tri = _scene_materials(meshes)
    if any(isinstance(m, MaterialEx) for m in table):
        table = [widen(m) for m in table]
    return table, tri


def _scene_materials(meshes):
    table, index, tri = [], {}, []
    for mesh in meshes:
        m = mesh[4] if len(mesh) > 4 else None
        k = -1
        if m is not None:
            if id(m) not in index:
                index[id(m)] = len(table)
                table.append(m)
            k = index[id(m)]
        tri += [k] * (len(mesh[1]) // 3)
    return table, tri


MATERIAL_INTERFACE = 3
MAX_MEDIA = 64


def interface() -> Material:
    """Material "" / "none": no BSDF, both walks pass through (a medium boundary).  A context takes it only
    after BeamGather.set_media."""
    return Material(MATERIAL_INTERFACE, _rgb(0.0), _rgb(0.0), 0.0)


class Medium(ctypes.Structure):
    """bre_medium: a HomogeneousMedium or a GridDensityMedium of the context's media table (120 bytes)."""
    _fields_ = [("type", ctypes.c_int32), ("sigma_a", F3), ("sigma_s", F3), ("g", ctypes.c_float),
                ("grid_n", ctypes.c_int32 * 3), ("world_to_medium", ctypes.c_float * 16),
                ("reserved", ctypes.c_int32), ("grid_density", ctypes.c_void_p)]

    def to_bytes(self) -> bytes:
        return ctypes.string_at(ctypes.addressof(self), ctypes.sizeof(self))


def medium_homogeneous(sigma_a, sigma_s, g: float = 0.0) -> Medium:
    """MakeNamedMedium "homogeneous": sigma_a, sigma_s (rgb or scalar, "scale" applied), HG g."""
    m = Medium()
    m.type = MEDIUM_HOMOGENEOUS
    m.sigma_a, m.sigma_s, m.g = _rgb(sigma_a), _rgb(sigma_s), float(g)
    return m


def medium_grid(sigma_a, sigma_s, g, density, n, world_to_medium=None) -> Medium:
    """MakeNamedMedium "heterogeneous": a GridDensityMedium over `density` (n = (nx, ny, nz) or int, x fastest)
    on the medium-space unit cube.  The array is kept alive on the object (the struct holds its address)."""
    import numpy as np

    nx, ny, nz = (n, n, n) if isinstance(n, int) else tuple(n)
    dens = np.ascontiguousarray(density, np.float32).reshape(-1)
    assert dens.shape[0] == nx * ny * nz
    m = medium_homogeneous(sigma_a, sigma_s, g)
    m.type = MEDIUM_GRID
    m.grid_n = (ctypes.c_int32 * 3)(nx, ny, nz)
    w = np.eye(4, dtype=np.float32) if world_to_medium is None else np.asarray(world_to_medium, np.float32)
    m.world_to_medium = (ctypes.c_float * 16)(*[float(v) for v in w.reshape(-1)])
    m.grid_density = dens.ctypes.data
    m._density_ref = dens
    return m


def scene_media(meshes, camera_medium=None, light_media=()):
    """(media, tri_inside, tri_outside, camera_medium, light_medium) of `meshes` for BeamGather.set_media.  A
    mesh's sixth element is its MediumInterface, a pair (inside, outside) of Medium objects or None (vacuum);
    a mesh without one is no transition (-1, -1).  `camera_medium` and `light_media` (one per delta light)
    are Medium objects or None.  One table entry per distinct Medium object, in order of first use."""
    table, index = [], {}

    def idx(m):
        if m is None:
            return -1
        if id(m) not in index:
            index[id(m)] = len(table)
            table.append(m)
        return index[id(m)]

    inside, outside = [], []
    for mesh in meshes:
        pair = mesh[5] if len(mesh) > 5 and mesh[5] is not None else (None, None)
        k = len(mesh[1]) // 3
        inside += [idx(pair[0])] * k
        outside += [idx(pair[1])] * k
    return table, inside, outside, idx(camera_medium), [idx(m) for m in light_media]


class RenderParams(ctypes.Structure):
    """bre_render_params: CreatePhotonBeamIntegrator's parameters (photonbeam.cpp:589-611)."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("iterations", ctypes.c_int32),
                ("start_iteration", ctypes.c_int32), ("end_iteration", ctypes.c_int32),
                ("photons_per_iteration", ctypes.c_int64), ("max_depth", ctypes.c_int32),
                ("render_surfaces", ctypes.c_int32), ("render_media", ctypes.c_int32),
                ("initial_radius", ctypes.c_float), ("alpha", ctypes.c_float)]


def render_params(width, height, iterations=64, photons=-1, max_depth=5, radius=1.0, alpha=0.5,
                  render_surfaces=True, render_media=True, start_iteration=0, end_iteration=None) -> RenderParams:
    """Defaults as the reference's (iterations 64, maxdepth 5, initialbeamradius 1, alpha 0.5)."""
    return RenderParams(int(width), int(height), int(iterations), int(start_iteration),
                        int(iterations if end_iteration is None else end_iteration), int(photons), int(max_depth),
                        int(render_surfaces), int(render_media), float(radius), float(alpha))


def _f3(v):
    return F3(*[float(x) for x in v])


def make_scene(meshes, sigma_a=None, sigma_s=None, g=0.0,
               cam_pos=(0.5, 0.5, 0.02), cam_look=(0.5, 0.5, 1.0), cam_up=(0.0, 1.0, 0.0), fov=60.0) -> Scene:
    """meshes: list of (P, indices, kd, Le) -- a pbrt "trianglemesh" with world-space points P
    (list of xyz), index triples, Lambertian kd, and Le (None = not emitting; two_sided(Le) = an
    AreaLightSource with "bool twosided" "true"); medium present iff
    sigma_a is given (RGB or scalar).  More than MAX_TRIANGLES triangles go to an external array
    (Scene.triangles_ext, kept alive on the scene object).  A mesh may carry a fifth element, its
    Material (mirror / glass) or None: the struct does not hold it (scene_materials(meshes) returns
    what BeamGather.set_materials takes).  A sixth element is the mesh's MediumInterface, a pair (inside,
    outside) of Medium objects or None (scene_media(meshes, ...) returns what BeamGather.set_media takes)."""
    s = Scene()
    ctypes.memset(ctypes.addressof(s), 0, ctypes.sizeof(s))
    total = sum(len(mesh[1]) // 3 for mesh in meshes)
    assert total <= MAX_SCENE_TRIANGLES
    ext = (Triangle * total)() if total > MAX_TRIANGLES else None
    dst = ext if ext is not None else s.triangles
    n = 0
    for P, idx, kd, Le in (mesh[:4] for mesh in meshes):
        assert len(idx) % 3 == 0
        for t in range(len(idx) // 3):
            T = dst[n]
            for v in range(3):
                T.p[v] = _f3(P[idx[3 * t + v]])
            T.kd = _f3(kd)
            if Le is not None:
                T.emit = EMIT_TWO_SIDED if isinstance(Le, two_sided) else EMIT_ONE_SIDED
                T.Le = _f3(Le)
            n += 1
    s.n_triangles = n
    if ext is not None:
        s.triangles_ext = ctypes.addressof(ext)
        s._triangles_ref = ext
    if sigma_a is not None:
        rgb = (lambda v: (v, v, v) if isinstance(v, (int, float)) else tuple(v))
        s.has_medium = 1
        s.sigma_a = _f3(rgb(sigma_a))
        s.sigma_s = _f3(rgb(sigma_s))
        s.g = float(g)
    s.cam_pos, s.cam_look, s.cam_up = _f3(cam_pos), _f3(cam_look), _f3(cam_up)
    s.cam_fov_deg = float(fov)
    return s


WHITE = (0.73, 0.73, 0.73)
RED = (0.63, 0.065, 0.05)
GREEN = (0.14, 0.45, 0.091)
QUAD = (0, 1, 2, 0, 2, 3)  # scenes/cornell_world.pbrt: "integer indices" [0 1 2 0 2 3]


def cornell_meshes(light_L=(17.0, 12.0, 4.0)):
    """scenes/cornell_world.pbrt: unit-cube Cornell box, one two-triangle mesh per wall (normals
    inward), the area light last (facing down)."""
    return [
        ([(0, 0, 0), (0, 0, 1), (1, 0, 1), (1, 0, 0)], QUAD, WHITE, None),     # floor
        ([(0, 1, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1)], QUAD, WHITE, None),     # ceiling
        ([(0, 0, 1), (0, 1, 1), (1, 1, 1), (1, 0, 1)], QUAD, WHITE, None),     # back wall
        ([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], QUAD, WHITE, None),     # front wall (behind the camera)
        ([(0, 0, 0), (0, 1, 0), (0, 1, 1), (0, 0, 1)], QUAD, RED, None),       # left wall
        ([(1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0)], QUAD, GREEN, None),     # right wall
        ([(0.35, 0.999, 0.35), (0.65, 0.999, 0.35), (0.65, 0.999, 0.65), (0.35, 0.999, 0.65)], QUAD, (0, 0, 0),
         light_L),                                                            # area light
    ]


def cornell_scene(sigma_a: float = 0.05, sigma_s: float = 0.5, g: float = 0.0) -> Scene:
    """Cornell box in homogeneous fog (sigma_a 0.05, sigma_s 0.5, g 0)."""
    return make_scene(cornell_meshes(), sigma_a, sigma_s, g)


def uv_sphere(center=(0.5, 0.35, 0.55), radius=0.2, n_theta=64, n_phi=96):
    """A triangulated sphere as one pbrt "trianglemesh": (points, indices) with n_theta rings and
    n_phi segments, outward-facing (counter-clockwise seen from outside), poles shared:
    2 * n_phi * (n_theta - 1) triangles (12,096 at the defaults)."""
    import numpy as np

    cx, cy, cz = (float(v) for v in center)
    pts = [(cx, cy + radius, cz)]
    for t in range(1, n_theta):
        th = np.pi * t / n_theta
        for k in range(n_phi):
            ph = 2 * np.pi * k / n_phi
            pts.append((cx + radius * np.sin(th) * np.cos(ph), cy + radius * np.cos(th), cz + radius * np.sin(th) * np.sin(ph)))
    pts.append((cx, cy - radius, cz))
    ring = lambda t, k: 1 + (t - 1) * n_phi + (k % n_phi)  # noqa: E731
    idx = []
    for k in range(n_phi):
        idx += [0, ring(1, k + 1), ring(1, k)]
    for t in range(1, n_theta - 1):
        for k in range(n_phi):
            a, b, c, d = ring(t, k), ring(t, k + 1), ring(t + 1, k), ring(t + 1, k + 1)
            idx += [a, b, d, a, d, c]
    south = len(pts) - 1
    for k in range(n_phi):
        idx += [south, ring(n_theta - 1, k), ring(n_theta - 1, k + 1)]
    return [tuple(np.float32(c) for c in p) for p in pts], idx


def cornell_sphere_scene(sigma_a: float = 0.05, sigma_s: float = 0.5, g: float = 0.0, n_theta=64, n_phi=96) -> Scene:
    """The C1/C2 Cornell box in fog with a white tessellated sphere (uv_sphere, 12,096 triangles at
    the defaults) on the floor side: a scene far past the 128 inline triangles, through
    Scene.triangles_ext and the scene BVH (bvh.cpp BVHAccel)."""
    P, idx = uv_sphere(n_theta=n_theta, n_phi=n_phi)
    meshes = cornell_meshes()
    return make_scene(meshes[:-1] + [(P, idx, (0.6, 0.6, 0.6), None)] + meshes[-1:], sigma_a, sigma_s, g)


def smoke_density(n: int = 64, seed: int = 7):
    """bre_smoke_density: seeded value-noise smoke (n^3 float32, x fastest), from libbre's host code."""
    import numpy as np

    from . import load_library

    lib = load_library()
    out = np.zeros(n * n * n, np.float32)
    lib.bre_smoke_density(ctypes.c_int32(n), ctypes.c_uint64(seed), out.ctypes.data_as(ctypes.c_void_p))
    return out


def grid_medium(scene: Scene, density, n, world_to_medium=None) -> Scene:
    """Turn `scene`'s medium into a GridDensityMedium over `density` (n = (nx, ny, nz) or int).
    The array is kept alive on the scene object (the struct only holds its address)."""
    import numpy as np

    nx, ny, nz = (n, n, n) if isinstance(n, int) else tuple(n)
    dens = np.ascontiguousarray(density, np.float32).reshape(-1)
    assert dens.shape[0] == nx * ny * nz
    scene.has_medium = MEDIUM_GRID
    scene.grid_n = (ctypes.c_int32 * 3)(nx, ny, nz)
    m = np.eye(4, dtype=np.float32) if world_to_medium is None else np.asarray(world_to_medium, np.float32)
    scene.world_to_medium = (ctypes.c_float * 16)(*[float(v) for v in m.reshape(-1)])
    scene.grid_density = dens.ctypes.data
    scene._density_ref = dens
    return scene


def cornell_smoke_scene(sigma_a: float = 0.5, sigma_s: float = 4.5, g: float = 0.7, n: int = 64, seed: int = 7,
                        density=None) -> Scene:
    """the Cornell box filled (on its unit cube) with a GridDensityMedium of
    seeded value-noise smoke (bre_smoke_density(n, seed)), spectrally uniform sigma_t, HG g."""
    s = cornell_scene(sigma_a, sigma_s, g)
    return grid_medium(s, smoke_density(n, seed) if density is None else density, n)
