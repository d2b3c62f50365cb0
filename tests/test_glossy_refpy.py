"""The plastic / metal / Oren-Nayar oracle on the CPU: tests/refpy_bsdf.py and tests/refpy_passes_bsdf.py.

1. refpy_passes_bsdf (a BSDF object per triangle) equals refpy_passes (the hand-chosen lobes) bit for bit on the
   existing scenes: this pins the restated loops.
2. Identities inside the new oracle: a one-lobe plastic and a sigma-0 matte entry are the triangle's own kd.
3. Known answers for the lobes, hand-derived and statistical.
4. Every branch counter of refpy_bsdf reaches 20 over the scenes of tests/glossy_scenes.py.
5. The midpoint margin of every normal-incidence sample the bit-exact GPU tests take, and
   the error of include/bre_fmath.h's bre_sincos_2pi against the host libm.
6. The record's size and the Python view's round trip.
"""
import ctypes
import importlib
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import glossy_lobes as gl
import glossy_refs as gr
import glossy_scenes as gs
import lights_scenes
import media_scenes
import pass_refs
import refpy_bsdf as rb
import refpy_passes_bsdf as rpb
import refpy_specular as rs
import specular_scenes
from refpy_photon import RNG, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEAM_KEYS = ("start", "end", "radius", "power", "counts")
SEG_KEYS = ("o", "p", "d", "tmax", "pixel", "depth", "surface")
DEEP_NAMES = ("plastic", "mixed")  # the scenes test_glossy_gpu.py runs at maxdepth 16
E_MAX = 2.0 ** -48     # the largest error this change's specification allows the device's double sin / cos
E_DERIVED = 2.0 ** -50  # the bound derived in include/bre_fmath.h
MARGIN = 2.0 ** -46    # 4 * E_MAX


def same(a, b, keys):
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape, k
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                              y.view(np.uint32) if y.dtype == np.float32 else y), k


# ---------------- 1. the restated loops ----------------
EXISTING = ([(specular_scenes, n) for n in specular_scenes.NAMES] + [(media_scenes, n) for n in media_scenes.NAMES] +
            [(lights_scenes, "mixed")])
EXISTING_CAMERA = EXISTING  # every scene for both passes (specular_scenes' own camera tests leave eta1 out)
_id = lambda v: f"{v[0].__name__}-{v[1]}"  # noqa: E731


@pytest.mark.parametrize("case", EXISTING, ids=_id)
def test_photon_pass_equals_refpy_passes(case):
    mod, name = case
    ref, _ = pass_refs.photon_ref(mod, name, 0)
    got = rpb.trace_photons(rpb.Scene(*mod.build(name)), mod.N_PHOTONS, 0, mod.MAX_DEPTH, mod.RADIUS)
    assert got["counts"].sum() > mod.N_PHOTONS // 2
    same(got, ref, BEAM_KEYS)


@pytest.mark.parametrize("case", EXISTING_CAMERA, ids=_id)
def test_camera_pass_equals_refpy_passes(case):
    mod, name = case
    ref, _ = pass_refs.camera_ref(mod, name, 0)
    got = rpb.camera_pass(rpb.Scene(*mod.build(name)), mod.CAM_W, mod.CAM_H, 0, mod.CAM_DEPTH)
    assert got["o"].shape[0] > 0
    same(got, ref, SEG_KEYS)


# ---------------- 2. one lobe is the lobe ----------------
def test_onelobe_is_the_triangles_own_kd():
    a, b = gs.build("onelobe"), gs.build("onelobe_plain")
    assert a.tri_mat != b.tri_mat and len(a.materials) == 4 and len(b.materials) == 2
    pa, _, _ = gr.photon_ref("onelobe", 0)
    pb = rpb.trace_photons(gr.scene("onelobe_plain"), gs.N_PHOTONS, 0, gs.MAX_DEPTH, gs.RADIUS)
    same(pa, pb, BEAM_KEYS)
    ca, _, _ = gr.camera_ref("onelobe", 0)
    cb = rpb.camera_pass(gr.scene("onelobe_plain"), gs.CAM_W, gs.CAM_H, 0, gs.CAM_DEPTH)
    assert ca["surface"].max() > 0
    same(ca, cb, SEG_KEYS)
    # the no-BxDF plastic ends a path like a black kd
    assert gr.scene("onelobe").bsdf[10].none and gr.scene("onelobe").bsdf[11].none


# ---------------- 3. known answers ----------------
def _dir(theta, phi=0.3):
    return (f32(math.sin(theta) * math.cos(phi)), f32(math.sin(theta) * math.sin(phi)), f32(math.cos(theta)))


def test_lobe_known_answers():
    Z = (f32(0), f32(0), f32(1))
    for ax, ay in ((0.1, 0.1), (0.05, 0.4), (1.0, 1.0)):
        d = rb.tr_D(f32(ax), f32(ay), Z)  # tan2 = 0: 1 / (pi ax ay)
        assert abs(float(d) - 1 / (math.pi * float(f32(ax)) * float(f32(ay)))) <= 4 * 2.0 ** -24 * float(d)
        assert rb.tr_lambda(f32(ax), f32(ay), Z) == 0
        assert rb.tr_G1(f32(ax), f32(ay), Z) == 1
    # FrConductor at k = 0 is FrDielectric (both in float32: a few ulps of the larger terms apart)
    for eta in (1.3, 1.5, 2.4):
        for c in (1.0, 0.9, 0.5, 0.2, 0.05):
            fd = float(rs.fr_dielectric(f32(c), f32(1), f32(eta))[0])
            fc = float(rb.fr_conductor(f32(c), f32(eta), f32(0)))
            assert abs(fc - fd) <= 1e-5, (eta, c, fc, fd)
    # Oren-Nayar towards sigma 0 is R / pi
    b = rb.Bsdf(rb.MATTE, kd=(0.5, 0.25, 1.0), sigma=1e-3)
    assert b.lobes == [rb.OREN]
    f = b.f(rb.FRAME, _dir(0.7, 0.2), _dir(0.4, 2.0))
    for got, k in zip(f, (0.5, 0.25, 1.0)):
        assert abs(float(got) - k / math.pi) <= 1e-6
    assert rb.Bsdf(rb.MATTE, kd=(0.5, 0.5, 0.5), sigma=0.0).lobes == [rb.LAMBERT]
    # RoughnessToAlpha of the plastic default, and the material set-up
    x = math.log(float(f32(0.1)))
    poly = 1.62142 + 0.819955 * x + 0.1734 * x ** 2 + 0.0171201 * x ** 3 + 0.000640711 * x ** 4  # 0.46176
    assert abs(float(rb.roughness_to_alpha(0.1)) - poly) < 1e-6 and abs(poly - 0.46176) < 1e-5
    assert rb.roughness_to_alpha(1e-4) == rb.roughness_to_alpha(1e-3)  # std::max(roughness, 1e-3)
    p = rb.Bsdf(rb.PLASTIC, kd=(0.25,) * 3, ks=(0.25,) * 3)
    assert p.lobes == [rb.LAMBERT, rb.MICRO] and p.ax == p.ay == rb.roughness_to_alpha(0.1)
    m = rb.Bsdf(rb.METAL, ceta=(0.2, 0.9, 1.1), ck=(3.9, 2.4, 2.1), roughness=0.01, vroughness=0.4, remap=False)
    assert m.lobes == [rb.MICRO] and (m.ax, m.ay) == (f32(0.01), f32(0.4)) and m.ks == (1, 1, 1)


@pytest.mark.parametrize("alpha", [(0.1, 0.1), (0.4, 0.4), (1.0, 1.0), (0.05, 0.4)], ids=str)
def test_distribution_pdf_integrates_to_one(alpha):
    """MicrofacetDistribution::Pdf over the hemisphere of wh, seen from the normal (wo . wh >= 0 everywhere), by the
    midpoint rule in double: within 1 %."""
    ax, ay = f32(alpha[0]), f32(alpha[1])
    nt, nphi = 600, (8 if alpha[0] == alpha[1] else 96)
    wo = (f32(0), f32(0), f32(1))
    total = 0.0
    for i in range(nt):
        # nodes in t = tan(theta / 2)-like stretch would be finer; a uniform theta grid resolves alpha >= 0.05
        th = (i + 0.5) * (math.pi / 2) / nt
        ring = 0.0
        for j in range(nphi):
            ring += float(rb.tr_pdf(ax, ay, wo, _dir(th, (j + 0.5) * 2 * math.pi / nphi)))
        total += ring * math.sin(th)
    total *= (math.pi / 2) / nt * (2 * math.pi / nphi)
    assert abs(total - 1) <= 0.01, total


def test_sample_mean_equals_quadrature():
    """E[f cos / pdf] under BSDF::Sample_f is the hemisphere integral of f cos (one channel, in double).  The bound
    is four standard errors of the mean, estimated from the samples, plus 1 % for the quadrature."""
    b = rb.Bsdf(rb.PLASTIC, kd=(0.4,) * 3, ks=(0.6,) * 3, roughness=0.4, remap=False)
    wo = _dir(0.5, 0.0)
    nt, nphi = 64, 128
    quad = 0.0
    for i in range(nt):
        th = (i + 0.5) * (math.pi / 2) / nt
        ring = sum(float(b.f(rb.FRAME, wo, _dir(th, (j + 0.5) * 2 * math.pi / nphi))[0]) for j in range(nphi))
        quad += ring * math.sin(th) * math.cos(th)
    quad *= (math.pi / 2) / nt * (2 * math.pi / nphi)
    rng = RNG(7)
    vals = []
    for _ in range(4000):
        u0, u1 = rng.get2d()
        s = b.sample(rb.FRAME, wo, u0, u1)
        vals.append(0.0 if s is None else float(s[2][0]) * abs(float(s[0][2])) / float(s[1]))
    mean, sem = float(np.mean(vals)), float(np.std(vals) / math.sqrt(len(vals)))
    assert 0.3 < quad < 1.0
    assert abs(mean - quad) <= 4 * sem + 0.01 * quad, (mean, quad, sem)


# ---------------- 4. branch coverage ----------------
def _all_refs():
    for name in gs.NAMES:
        for it in gs.PHOTON_ITERATIONS:
            yield gr.photon_ref(name, it)
        for it in gs.CAMERA_ITERATIONS:
            yield gr.camera_ref(name, it)


def test_every_branch_counter_reaches_20():
    total = {k: 0 for k in rb.COUNTERS}
    for _, stats, _ in _all_refs():
        for k in total:
            total[k] += stats[k]
    print(total)
    for k, v in total.items():
        assert v >= 20, (k, total)


# ---------------- 5. the double branch ----------------
def test_midpoint_margin_of_every_normal_incidence_sample():
    """A condition on the inputs, checked on the reference alone: for every normal-incidence sample of the lobe
    records and of the pass references, the double products r cos(phi) and r sin(phi) lie at least 2^-46, relative,
    from a float32 rounding midpoint, four times the largest error the device's cos / sin may have.  About 0.03
    violations are expected in 60k samples; none of the records has had to be nudged."""
    samples = list(gl.reference()[2])
    for _, _, normals in _all_refs():
        samples += list(normals)
    for name in DEEP_NAMES:  # test_photon_pass_at_the_deepest_maxdepth's references
        samples += list(gr.deep_photon_ref(name, 16)[1])
    assert len(samples) > 8000
    worst = math.inf
    for r, phi in samples:
        for v in (float(r) * math.cos(float(phi)), float(r) * math.sin(float(phi))):
            worst = min(worst, rb.midpoint_margin(v))
    print(f"{len(samples)} normal-incidence samples, smallest margin 2^{math.log2(worst):.1f}")
    assert worst >= MARGIN


PI_60 = Fraction(3141592653589793238462643383279502884197169399375105820974944592, 10 ** 63)


@pytest.fixture(scope="module")
def sincos_2pi(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sincos") / "libfmath_sincos2pi.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fno-builtin", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "fmath_sincos2pi.c"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.fmath_sincos_2pi.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]

    def run(phi):
        phi = np.ascontiguousarray(phi, np.float64)
        s, c = np.zeros_like(phi), np.zeros_like(phi)
        lib.fmath_sincos_2pi(phi.ctypes.data, phi.size, s.ctypes.data, c.ctypes.data)
        return s, c

    return run


def test_double_sincos_error_bound(sincos_2pi):
    """bre_sincos_2pi on float arguments in [0, 2 pi] against the host libm (under 1 ulp = 2^-53 relative): within the
    derived E = 2^-50 plus libm's own ulp, on every float within 64 ulps of a multiple of pi/2, on the phi of every
    U2 of a dense grid, and at the ends.  The derivation's premise, that no float lies within 2^-27 of a non-zero
    multiple of pi/2, is checked exactly."""
    near = []
    for k in range(1, 5):
        c = np.float32(float(PI_60 * k / 2))
        lo = c
        for _ in range(64):
            lo = np.nextafter(lo, np.float32(0))
        v = lo
        for _ in range(129):
            near.append(v)
            d = abs(Fraction(float(v)) - PI_60 * k / 2)
            assert d >= Fraction(1, 2 ** 27), (k, float(v))
            v = np.nextafter(v, np.float32(10))
    u2 = np.concatenate([np.linspace(0, 1, 200001)[:-1], [0.99999994, 0.5, 0.25, 0.75, 1e-30, 1e-8]]).astype(np.float32)
    phi = np.concatenate([np.array(near, np.float32), (6.28318530718 * u2.astype(np.float64)).astype(np.float32)])
    assert phi.min() >= 0 and phi.max() < 6.2833  # the sampler's range, and the 64 floats past float(2 pi)
    s, c = sincos_2pi(phi.astype(np.float64))
    rs_ = np.array([math.sin(float(p)) for p in phi])
    rc_ = np.array([math.cos(float(p)) for p in phi])
    tol = E_DERIVED + 2.0 ** -53
    assert tol < E_MAX
    es = np.abs(s - rs_) / np.maximum(np.abs(rs_), 1e-300)
    ec = np.abs(c - rc_) / np.maximum(np.abs(rc_), 1e-300)
    es[rs_ == 0] = np.abs(s[rs_ == 0])
    print(f"largest relative difference from libm: sin 2^{math.log2(max(es.max(), 1e-300)):.1f}, "
          f"cos 2^{math.log2(max(ec.max(), 1e-300)):.1f}")
    assert es.max() <= tol and ec.max() <= tol


# ---------------- 6. the record ----------------
def test_material_ex_record_and_python_view():
    sm = importlib.import_module("beam-radiance-estimate-pbrt_amd.scene")
    assert ctypes.sizeof(sm.MaterialEx) == 112 and ctypes.sizeof(sm.Material) == 32
    header = open(os.path.join(ROOT, "include", "bre_scene.h")).read()
    assert "} bre_material_ex;" in header and "112 bytes" in header
    for name, _ in sm.Material._fields_:  # a superset: the narrow record is its first 32 bytes
        assert getattr(sm.MaterialEx, name).offset == getattr(sm.Material, name).offset
    g = sm.glass(0.9, 0.8, 1.33)
    w = sm.widen(g)
    assert w.to_bytes()[:32] == g.to_bytes() and w.to_bytes()[32:] == bytes(80) and sm.widen(w) is w
    p = sm.plastic((0.1, 0.2, 0.3), 0.4, 0.05, False)
    assert (p.type, tuple(p.kd), tuple(p.ks), p.roughness, p.remap) == (5, tuple(f32(x) for x in (0.1, 0.2, 0.3)),
                                                                        (f32(0.4),) * 3, f32(0.05), 0)
    m = sm.metal((0.2, 0.9, 1.1), 3.0, 0.01, vroughness=0.4)
    assert (m.type, tuple(m.ck), m.uroughness, m.vroughness, m.remap) == (6, (3.0,) * 3, 0.0, f32(0.4), 1)
    t = sm.matte(0.5, 20.0)
    assert (t.type, tuple(t.kd), t.sigma) == (4, (0.5,) * 3, 20.0)
    assert sm.MaterialEx.from_buffer_copy(p.to_bytes()).to_bytes() == p.to_bytes()
    # scene_materials: narrow tables stay narrow, one wide entry widens the whole table; equal objects share
    quad = ([(0, 0, 0), (0, 0, 1), (1, 0, 1), (1, 0, 0)], sm.QUAD, (0.5,) * 3, None)
    table, tri = sm.scene_materials([quad + (g,), quad, quad + (g,)])
    assert [type(x) for x in table] == [sm.Material] and tri == [0, 0, -1, -1, 0, 0]
    table, tri = sm.scene_materials([quad + (g,), quad + (p,), quad + (p,)])
    assert [type(x) for x in table] == [sm.MaterialEx] * 2 and tri == [0, 0, 1, 1, 1, 1]
    assert table[0].to_bytes()[:32] == g.to_bytes() and table[1] is p
    # the oracle's view of a record is the record
    b = rb.Bsdf.of(m)
    assert b.lobes == [rb.MICRO] and b.ceta == tuple(f32(x) for x in (0.2, 0.9, 1.1))


# ---------------- 7. the .pbrt front end ----------------
HEAD = """LookAt 0.5 0.5 0.02  0.5 0.5 1  0 1 0
Camera "perspective" "float fov" [60]
Film "image" "integer xresolution" [64] "integer yresolution" [48] "string filename" "x.pfm"
Integrator "photonbeam" "integer iterations" [3] "integer photonsperiteration" [20000]
WorldBegin
AttributeBegin
  Material "matte" "rgb Kd" [0 0 0]
  AreaLightSource "diffuse" "rgb L" [17 12 4]
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3]
      "point P" [0.35 0.999 0.35  0.65 0.999 0.35  0.65 0.999 0.65  0.35 0.999 0.65]
AttributeEnd
"""
FLOOR = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0 0 0  0 0 1  1 0 1  1 0 0]\n'
ETA_K = '"rgb eta" [0.2 0.9 1.1] "rgb k" [3.9 2.4 2.1]'


@pytest.fixture(scope="module")
def pb():
    return importlib.import_module("beam-radiance-estimate-pbrt_amd.pbrt")


@pytest.fixture(scope="module")
def sm():
    return importlib.import_module("beam-radiance-estimate-pbrt_amd.scene")


def test_glossy_fog_parses_to_the_hand_built_scene(pb, sm):
    s = pb.parse_file(os.path.join(ROOT, "scenes", "glossy_fog.pbrt"))
    assert s.ok and s.n_errors == 0, s.messages
    case = gs.build("glossy_fog")
    assert s.scene.n_triangles == case.scene.n_triangles == 14
    assert s.scene.to_bytes() == case.scene.to_bytes()
    assert [m.to_bytes() for m in s.materials_ex] == [m.to_bytes() for m in case.materials]
    assert [m.type for m in s.materials_ex] == [sm.MATERIAL_PLASTIC, sm.MATERIAL_MATTE, sm.MATERIAL_MATTE,
                                                sm.MATERIAL_MATTE, sm.MATERIAL_METAL]
    assert s.triangle_material.tolist() == list(case.tri_mat) == [0] * 2 + [1] * 6 + [2] * 2 + [3] * 2 + [4] * 2
    assert len(s.lights) == 1 and s.lights[0].to_bytes() == case.lights[0].to_bytes()
    # the narrow getter cannot express the scene: BRE_ERR_STATE, and the Python view falls back to the wide records
    assert s.materials_status == 4 and s.materials is s.materials_ex
    n = ctypes.c_int32()
    assert s._lib.bre_pbrt_get_materials(s._h, 0, None, ctypes.byref(n), 0, None, None) == 4 and n.value == 5


def test_glossy_material_statements(pb, sm):
    def parse(body):
        return pb.parse_string(HEAD + body + "WorldEnd\n")

    # defaults: plastic Kd 0.25, Ks 0.25, roughness 0.1, remapped; metal roughness 0.01 with no u / v given
    s = parse('Material "plastic"\n' + FLOOR + 'Material "metal" ' + ETA_K + '\n' + FLOOR)
    assert s.ok and s.n_errors == 0, s.messages
    assert [m.to_bytes() for m in s.materials_ex] == [sm.plastic().to_bytes(),
                                                      sm.metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.1)).to_bytes()]
    p, m = s.materials_ex
    assert (list(p.kd), list(p.ks), p.roughness, p.remap) == ([0.25] * 3, [0.25] * 3, f32(0.1), 1)
    assert (m.roughness, m.uroughness, m.vroughness, m.remap) == (f32(0.01), 0.0, 0.0, 1)
    assert s.triangle_material.tolist() == [-1, -1, 0, 0, 1, 1] and s.materials_status == 4
    assert bytes(s.scene.triangles[2].kd) == bytes(sm.F3(0.5, 0.5, 0.5))  # what a triangle under an entry keeps
    # the roughness fallback of metal: one of u / v given, the other falls back (in the record: 0)
    s = parse('Material "metal" ' + ETA_K + ' "float roughness" [0.2] "float vroughness" [0.4]\n' + FLOOR)
    assert s.n_errors == 0 and s.materials_ex[0].to_bytes() == sm.metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.1), 0.2, 0.0, 0.4).to_bytes()
    b = rb.Bsdf.of(s.materials_ex[0])
    assert (b.ax, b.ay) == (rb.roughness_to_alpha(0.2), rb.roughness_to_alpha(0.4))
    # "remaproughness" false, named materials, and matte with sigma as an entry whose triangles keep their Kd
    s = parse('MakeNamedMaterial "p" "string type" "plastic" "rgb Kd" [0.1 0.2 0.3] "rgb Ks" [0.4 0.5 0.6] '
              '"float roughness" [0.3] "bool remaproughness" "false"\n'
              'MakeNamedMaterial "m" "string type" "metal" ' + ETA_K + ' "float uroughness" [0.05] '
              '"float vroughness" [0.4] "bool remaproughness" "false"\nNamedMaterial "p"\n' + FLOOR +
              'NamedMaterial "m"\n' + FLOOR + 'Material "matte" "rgb Kd" [0.6 0.5 0.4] "float sigma" [20]\n' + FLOOR)
    assert s.ok and s.n_errors == 0, s.messages
    assert [x.to_bytes() for x in s.materials_ex] == [
        sm.plastic((0.1, 0.2, 0.3), (0.4, 0.5, 0.6), 0.3, False).to_bytes(),
        sm.metal((0.2, 0.9, 1.1), (3.9, 2.4, 2.1), 0.01, 0.05, 0.4, False).to_bytes(),
        sm.matte((0.6, 0.5, 0.4), 20.0).to_bytes()]
    assert list(s.scene.triangles[6].kd) == [f32(0.6), f32(0.5), f32(0.4)]
    # equal materials share an entry, across kinds of statement; a narrow entry beside them is widened
    s = parse('Material "plastic" "float roughness" [0.1]\n' + FLOOR + 'Material "mirror"\n' + FLOOR +
              'MakeNamedMaterial "p" "string type" "plastic"\nNamedMaterial "p"\n' + FLOOR +
              'Material "matte" "float sigma" [30]\n' + FLOOR + 'Material "matte" "float sigma" [30]\n' + FLOOR)
    assert s.n_errors == 0 and s.triangle_material.tolist() == [-1, -1, 0, 0, 1, 1, 0, 0, 2, 2, 2, 2]
    assert s.materials_ex[1].to_bytes() == sm.widen(sm.mirror(0.9)).to_bytes() and s.materials_status == 4
    # a matte with sigma 0 keeps the per-triangle kd path: no table, and the narrow getter serves the scene
    s = parse('Material "matte" "rgb Kd" [0.6 0.5 0.4] "float sigma" [0]\n' + FLOOR)
    assert s.ok and s.n_errors == 0 and s.materials == [] and s.materials_ex == [] and s.triangle_material.size == 0
    s = parse('Material "mirror"\n' + FLOOR)
    assert s.materials_status == 0 and s.materials[0].to_bytes() == sm.mirror(0.9).to_bytes()
    assert s.materials_ex[0].to_bytes() == sm.widen(sm.mirror(0.9)).to_bytes()


def test_glossy_material_refusals(pb):
    """Reported, and the statement falls back to matte: no table entry."""
    def parse(body):
        return pb.parse_string(HEAD + body + "WorldEnd\n")

    cases = {
        'Material "plastic" "texture Kd" "t"\n': 'plastic "Kd" must be an rgb or xyz value (textures are not supported)',
        'Material "plastic" "texture Ks" "t"\n': 'plastic "Ks" must be an rgb or xyz value (textures are not supported)',
        'Material "plastic" "texture roughness" "t"\n': 'plastic "roughness" must be a float (textures are not supported)',
        'Material "plastic" "texture bumpmap" "b"\n': 'plastic "bumpmap" is not supported',
        'Material "plastic" "float roughness" [0]\n': 'plastic "roughness" must be finite and > 0',
        'Material "metal"\n': 'metal needs explicit "rgb eta" and "rgb k" (the default copper spectra are not supported)',
        'Material "metal" "rgb eta" [0.2 0.9 1.1]\n': 'metal needs explicit "rgb eta" and "rgb k"',
        'Material "metal" "texture eta" "t" "rgb k" [3 2 2]\n': 'metal "eta" must be an rgb or xyz value (textures are not supported)',
        'Material "metal" ' + ETA_K + ' "texture bumpmap" "b"\n': 'metal "bumpmap" is not supported',
        'Material "metal" ' + ETA_K + ' "texture uroughness" "t"\n': 'metal "uroughness" must be a float (textures are not supported)',
        'Material "metal" ' + ETA_K + ' "float roughness" [0]\n': 'must be finite and > 0',
        'Material "metal" ' + ETA_K + ' "float uroughness" [-0.1]\n': 'must be finite and > 0',
        'Material "metal" "rgb eta" [0.2 0 1.1] "rgb k" [3 2 2]\n': 'metal "eta" must not be 0 in any channel',
        'MakeNamedMaterial "m" "string type" "metal"\nNamedMaterial "m"\n': 'the default copper spectra are not supported',
        'Material "matte" "texture sigma" "t"\n': 'matte "sigma" must be a float (textures are not supported)',
        'Material "uber"\n': 'Material "uber" is not supported (matte, plastic, metal, mirror, named glass); using "matte"',
        'Material "substrate"\n': 'Material "substrate" is not supported (matte, plastic, metal, mirror, named glass)',
        'Material "translucent"\n': 'Material "translucent" is not supported (matte, plastic, metal, mirror, named glass)',
    }
    for stmt, msg in cases.items():
        s = parse(stmt + FLOOR)
        assert s.ok and s.n_errors >= 1 and msg in s.messages, (stmt, s.messages)
        assert s.materials_ex == [] and s.triangle_material.size == 0, stmt
