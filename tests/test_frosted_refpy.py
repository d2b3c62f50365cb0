"""Rough glass, uber, translucent and substrate without a GPU: the restatement (tests/refpy_bsdf_full.py,
tests/refpy_passes_full.py) held to answers derived by hand, the conditions on it that keep the GPU tests from
passing vacuously, the midpoint margin of every normal-incidence sample those tests take, and the Python records.

1. Known answers of each new lobe at configurations with a closed form.
2. Every branch counter of the restatement reaches 20 over the scenes of tests/frosted_scenes.py.
3. The 2^-46 midpoint margin of DESIGN.md section 23, on the reference alone.
4. The record helpers of scene.py: the layout, the opacity accessor, the defaults of the Create...Material functions.
5. Every refusal of the setter's check of a record (bre_check_material_ex: no context, no device) with its message.
6. The .pbrt front end with BRE_PBRT_MATERIALS: the parser's records byte for byte against the Python helpers,
   scenes/frosted_fog.pbrt against its hand-built twin, every new refusal with its message, and the default parse's
   five pinned messages unchanged.
"""
import ctypes
import importlib
import math
import os

import numpy as np
import pytest

import frosted_lobes as fl
import frosted_refs as fr
import frosted_scenes as fs
import refpy_bsdf as rb
import refpy_bsdf_full as rf
import refpy_passes_full as rpf
from refpy_photon import f32

MARGIN = 2.0 ** -46  # 4 * the largest error of the device's cos / sin (tests/test_glossy_refpy.py)
Z = (f32(0), f32(0), f32(1))
MZ = (f32(0), f32(0), f32(-1))


@pytest.fixture(scope="module")
def sm():
    return importlib.import_module("beam-radiance-estimate-pbrt_amd.scene")


def close(a, b, rel=2e-6):
    return abs(float(a) - float(b)) <= rel * abs(float(b))


# ---------------- 1. known answers ----------------
@pytest.mark.parametrize("alpha", [0.1, 0.5])
def test_microfacet_transmission_straight_through(alpha):
    """wo = +z, wi = -z, etaA = 1, etaB = 1.5: eta = 1.5, wh = z, D = 1 / (pi a^2), G = 1, F = 0.04,
    sqrtDenom = 1 - 1.5 = -0.5, so f = 0.96 T * 9 D in Importance and 0.96 T * 4 D in Radiance (factor 1 / eta), and
    Pdf = D * dwh_dwi = 9 D."""
    T = (f32(1), f32(0.5), f32(0.25))
    lobe = rf.MicrofacetTransmission(T, alpha, alpha, 1, 1.5)
    D = 1 / (math.pi * alpha * alpha)
    for mode, k in ((rf.IMPORTANCE, 9.0), (rf.RADIANCE, 4.0)):
        f = lobe.f(Z, MZ, mode)
        for c in range(3):
            assert close(f[c], 0.96 * float(T[c]) * k * D), (mode, f)
    assert close(lobe.pdf(Z, MZ), 9 * D)
    assert lobe.f(Z, Z, rf.RADIANCE) == rf.ZERO3 and lobe.pdf(Z, Z) == 0  # transmission only
    # from inside: eta = 1 / 1.5, sqrtDenom = -1 + 1 / 1.5; Importance f = 0.96 T D eta^2 / sd^2 = 0.96 T * 4 D
    f = lobe.f(MZ, Z, rf.IMPORTANCE)
    assert close(f[0], 0.96 * 4 * D) and close(lobe.f(MZ, Z, rf.RADIANCE)[0], 0.96 * 9 * D)


def test_fresnel_blend_at_normal_incidence():
    """wo = wi = z: diffuse = 28 / (23 pi) Rd (1 - Rs) (1 - 2^-5)^2, specular = D / 4 * Rs (Schlick's pow5(0) = 0),
    Pdf = (1 / pi + D / 4) / 2."""
    Rd, Rs, a = (f32(0.5), f32(0.25), f32(0)), (f32(0.5), f32(0.25), f32(1)), 0.2
    lobe = rf.FresnelBlend(Rd, Rs, a, a)
    D = 1 / (math.pi * a * a)
    f = lobe.f(Z, Z, rf.RADIANCE)
    for c in range(3):
        want = 28 / (23 * math.pi) * float(Rd[c]) * (1 - float(Rs[c])) * (1 - 2.0 ** -5) ** 2 + D / 4 * float(Rs[c])
        assert close(f[c], want), (c, f)
    assert close(lobe.pdf(Z, Z), 0.5 * (1 / math.pi + D / 4))
    assert lobe.pdf(Z, MZ) == 0
    # both halves of Sample_f: u0 < .5 is the cosine lobe with u0 doubled, the other the microfacet with 2 (u0 - .5)
    st = rf.new_stats()
    wo = (f32(0.6), f32(0), f32(0.8))
    a_, b_ = lobe.sample(wo, f32(0.25), f32(0.3), rf.RADIANCE, st), lobe.sample(wo, f32(0.75), f32(0.3), rf.RADIANCE, st)
    assert st["blend_diffuse_half"] == 1 and st["blend_specular_half"] == 1
    assert a_[0] == rf.LambertianReflection(Rd).sample(wo, f32(0.5), f32(0.3), rf.RADIANCE)[0]
    assert b_[0] == rf.MicrofacetReflection(Rd, a, a, 1, 1.5).sample(wo, f32(0.5), f32(0.3), rf.RADIANCE)[0]


def test_uber_with_opacity_zero_is_a_pass_through(sm):
    """opacity 0: one SpecularTransmission(1, 1, 1).  Refract with eta 1 returns -wo up to the rounding of
    cosThetaT, F = 0, pdf = 1, f |cos| = 1 in both modes; f() and Pdf() are 0, and EstimateDirect's flags match
    no lobe."""
    b = rf.FullBsdf.of(sm.uber(0.5, 0.5, 0.5, 0.5, opacity=0.0))
    assert [type(x) for x in b.lobes] == [rf.SpecularTransmission]
    for wo in ((0.6, 0.0, 0.8), (-0.3, 0.4, -math.sqrt(0.75))):
        wo = tuple(f32(v) for v in wo)
        for mode in (rf.IMPORTANCE, rf.RADIANCE):
            wi, pdf, f, typ = b.sample(rb.FRAME, wo, 0.3, 0.7, rf.BSDF_ALL, mode)
            assert pdf == 1 and typ == rf.BSDF_SPECULAR | rf.BSDF_TRANSMISSION
            assert all(abs(float(wi[k]) + float(wo[k])) < 1e-6 for k in range(3))
            assert all(close(float(f[c]) * abs(float(wi[2])), 1.0) for c in range(3))
        assert b.sample(rb.FRAME, wo, 0.3, 0.7, rf.BSDF_NON_SPECULAR, rf.RADIANCE) is None
        assert b.f(rb.FRAME, wo, tuple(-v for v in wo)) == rf.ZERO3 and b.pdf(rb.FRAME, wo, tuple(-v for v in wo)) == 0


def test_specular_lobes_under_a_dielectric():
    """Normal incidence between 1 and 1.5: F = 0.04.  SpecularReflection returns F R / |cos|, SpecularTransmission
    T (1 - F) / |cos|, times (etaI / etaT)^2 in Radiance only."""
    R = (f32(1), f32(0.5), f32(0))
    wi, pdf, f = rf.SpecularReflection(R, 1, 1.5).sample(Z, 0, 0, rf.RADIANCE)
    assert wi == (-Z[0], -Z[1], Z[2]) and pdf == 1 and close(f[0], 0.04) and close(f[1], 0.02) and f[2] == 0
    t = rf.SpecularTransmission(R, 1, 1.5)
    wi, pdf, f = t.sample(Z, 0, 0, rf.IMPORTANCE)
    assert tuple(float(v) for v in wi) == (0, 0, -1) and pdf == 1 and close(f[0], 0.96)
    assert close(t.sample(Z, 0, 0, rf.RADIANCE)[2][0], 0.96 / 2.25)
    assert close(t.sample(MZ, 0, 0, rf.RADIANCE)[2][0], 0.96 * 2.25)
    st = rf.new_stats()  # from inside beyond the critical angle: Refract fails, pdf stays 0
    s = math.sin(math.radians(60))
    assert t.sample((f32(s), f32(0), f32(-0.5)), 0, 0, rf.RADIANCE, st)[1] == 0 and st["tir_spec_t"] == 1


def test_lambertian_transmission_and_the_reflect_transmit_split(sm):
    """A translucent with Ks black: LambertianReflection(r kd) and LambertianTransmission(t kd).  BSDF::f takes the
    first on the reflecting side of the geometric normal and the second on the other; Pdf averages both lobes'."""
    b = rf.FullBsdf.of(sm.translucent((0.5, 0.4, 0.3), 0.0, 0.6, 0.4))
    assert [type(x) for x in b.lobes] == [rf.LambertianReflection, rf.LambertianTransmission]
    wo, up, down = (f32(0.6), f32(0), f32(0.8)), (f32(0), f32(0.6), f32(0.8)), (f32(0), f32(0.6), f32(-0.8))
    assert close(b.f(rb.FRAME, wo, up)[0], 0.6 * 0.5 / math.pi) and close(b.f(rb.FRAME, wo, down)[0], 0.4 * 0.5 / math.pi)
    assert close(b.pdf(rb.FRAME, wo, up), 0.8 / math.pi / 2) and close(b.pdf(rb.FRAME, wo, down), 0.8 / math.pi / 2)
    below = b.sample(rb.FRAME, wo, 0.75, 0.3)  # the second of two lobes
    assert below[0][2] < 0 and below[3] == rf.BSDF_TRANSMISSION | rf.BSDF_DIFFUSE
    assert close(below[1], abs(float(below[0][2])) / math.pi / 2) and close(below[2][1], 0.4 * 0.4 / math.pi)


def test_lobe_lists_flags_and_early_returns(sm):
    five = rf.FullBsdf.of(fl.materials()[4])
    assert [type(x).__name__ for x in five.lobes] == ["SpecularTransmission", "LambertianReflection",
                                                       "MicrofacetReflection", "SpecularReflection",
                                                       "SpecularTransmission"]
    assert len(five.matching(rf.BSDF_ALL)) == 5 and len(five.matching(rf.BSDF_NON_SPECULAR)) == 2
    assert float(five.lobes[0].T[0]) == float(f32(f32(-f32(0.6)) + f32(1)))  # 1 - opacity
    assert float(five.lobes[1].R[1]) == float(f32(f32(0.7) * f32(0.3)))      # op * Kd
    # a specular sample of a mixed BSDF: its own pdf over the five components, its own f, no sum
    wo = (f32(0.6), f32(0), f32(0.8))
    s = five.sample(rb.FRAME, wo, 0.05, 0.5, rf.BSDF_ALL, rf.RADIANCE)
    assert s[3] & rf.BSDF_SPECULAR and s[1] == f32(f32(1) / f32(5))
    assert float(s[2][0]) == float(five.lobes[0].sample(wo, f32(0.25), f32(0.5), rf.RADIANCE)[2][0])
    # a non-specular one: the specular lobes add nothing to the pdf but count in the division
    s = five.sample(rb.FRAME, wo, 0.3, 0.5, rf.BSDF_ALL, rf.RADIANCE)
    assert s[3] == rf.BSDF_REFLECTION | rf.BSDF_DIFFUSE
    lam, mic = five.lobes[1], five.lobes[2]
    wi = rb._to_local(rb.FRAME, s[0])
    assert s[1] == f32(f32(lam.pdf(wo, wi) + mic.pdf(wo, wi)) / f32(5))
    s2 = five.sample(rb.FRAME, wo, 0.3, 0.5, rf.BSDF_NON_SPECULAR, rf.RADIANCE)  # u0 * 2 = 0.6: the first of two
    assert s2[3] == s[3] and s2[1] != s[1]
    # the early returns and the uber fallbacks
    assert rf.FullBsdf.of(sm.translucent(0.5, 0.5, 0.0, 0.0)).none and rf.FullBsdf.of(sm.substrate(0.0, 0.0)).none
    assert rf.FullBsdf.of(sm.rough_glass(0.0, 0.0, 1.5, 0.1, 0.1)).none and rf.FullBsdf.of(sm.uber(0, 0, 0, 0)).none
    u = rf.FullBsdf.of(sm.uber(0.0, 0.5, 0.0, 0.0, 0.2, 0.05, 0.0, 1.5, 1.0, False)).lobes[0]
    assert (float(u.ax), float(u.ay)) == (float(f32(0.05)), float(f32(0.05)))  # roughv falls back to roughu
    u = rf.FullBsdf.of(sm.uber(0.0, 0.5, roughness=0.2, vroughness=0.4, remap=False)).lobes[0]
    assert (float(u.ax), float(u.ay)) == (float(f32(0.2)), float(f32(0.4)))
    g = rf.FullBsdf.of(sm.rough_glass(1.0, 1.0, 1.5, 0.0, 0.3, True)).lobes[1]
    assert float(g.ax) == float(rb.roughness_to_alpha(f32(1e-3))) > 0  # RoughnessToAlpha clamps at 1e-3


# ---------------- 2. conditions on the references ----------------
def _all_refs():
    for name in fs.NAMES:
        for it in fs.PHOTON_ITERATIONS:
            ref, tags, stats, normals = fr.photon_ref(name, it)
            yield stats, normals
        for it in fs.CAMERA_ITERATIONS:
            ref, info, stats, normals = fr.camera_ref(name, it)
            yield stats, normals


def test_every_branch_of_the_restatement_is_reached():
    """Over the scenes, each new counter reaches 20: each lobe chosen, total internal reflection in Refract for both
    lobe kinds, wh.z < 0 flipped, both halves of FresnelBlend::Sample_f, the !SameHemisphere returns, a specular
    and a non-specular sample from one BSDF, matchingComps == 0 in EstimateDirect, a transmitted light sample.
    (`no_matching_lobe`, BSDF::Sample_f's own matchingComps == 0, is reached by the lobe records instead: in the
    walks a BSDF without a BxDF ends the path before Sample_f, and EstimateDirect's case is counted by its own
    name.)"""
    total = rpf.new_stats()
    for stats, _ in _all_refs():
        for k in total:
            total[k] += stats[k]
    new = [k for k in rpf.COUNTERS if k not in rpf.rd.COUNTERS and k != "no_matching_lobe"]
    assert len(new) == 22
    print({k: total[k] for k in new})
    for k in new:
        assert total[k] >= 20, (k, total[k])
    assert fl.reference()[1]["no_matching_lobe"] >= 20
    assert sum(len(fr.camera_ref(n, i)[1]["le_after_uber_specular"]) for n in fs.NAMES for i in fs.CAMERA_ITERATIONS) >= 3


def test_scenes_stay_small_and_hold_the_new_types(sm):
    seen = set()
    for name in fs.NAMES:
        case = fs.build(name)
        assert case.scene.n_triangles <= 40
        seen |= {m.type for m in case.materials}
    assert {8, 9, 10, 11, sm.MATERIAL_PLASTIC, sm.MATERIAL_MIRROR} <= seen


# ---------------- 3. the double branch ----------------
def test_midpoint_margin_of_every_normal_incidence_sample():
    """For every normal-incidence sample of the lobe records and of the pass references, r cos(phi) and r sin(phi)
    in double lie at least 2^-46, relative, from a float32 rounding midpoint."""
    samples = list(fl.reference()[2])
    for _, normals in _all_refs():
        samples += list(normals)
    for name in fs.DEEP_NAMES:
        samples += list(fr.deep_photon_ref(name, 16)[1])
    assert len(samples) > 5000
    worst = math.inf
    for r, phi in samples:
        for v in (float(r) * math.cos(float(phi)), float(r) * math.sin(float(phi))):
            worst = min(worst, rb.midpoint_margin(v))
    print(f"{len(samples)} normal-incidence samples, smallest margin 2^{math.log2(worst):.1f}")
    assert worst >= MARGIN


# ---------------- 4. the Python records ----------------
def test_material_ex_records(sm):
    assert ctypes.sizeof(sm.MaterialEx) == 112 and sm.MaterialEx.ceta.offset == 56 and sm.MaterialEx.reserved.offset == 100
    assert (sm.MATERIAL_ROUGH_GLASS, sm.MATERIAL_UBER, sm.MATERIAL_TRANSLUCENT, sm.MATERIAL_SUBSTRATE) == (8, 9, 10, 11)
    u = sm.uber()  # CreateUberMaterial's defaults, uber.cpp:103-127
    assert (u.type, tuple(u.kd), tuple(u.ks), tuple(u.kr), tuple(u.kt)) == (9, (0.25,) * 3, (0.25,) * 3, (0,) * 3, (0,) * 3)
    assert (u.eta, u.uroughness, u.vroughness, u.remap, tuple(u.opacity)) == (1.5, 0, 0, 1, (1,) * 3)
    assert abs(u.roughness - 0.1) < 1e-8 and tuple(u.ceta) == tuple(u.opacity) and tuple(u.reserved) == (0, 0, 0)
    u.opacity = sm.F3(0.5, 0.25, 0.125)
    assert tuple(u.ceta) == (0.5, 0.25, 0.125)  # the record's anonymous union
    t = sm.translucent()  # translucent.cpp:82-98: reflect in kr, transmit in kt
    assert (t.type, tuple(t.kd), tuple(t.ks), tuple(t.kr), tuple(t.kt), t.remap) == (10, (0.25,) * 3, (0.25,) * 3, (0.5,) * 3, (0.5,) * 3, 1)
    assert (t.eta, tuple(t.ceta), t.uroughness) == (0, (0,) * 3, 0)
    s = sm.substrate()  # substrate.cpp:67-81
    assert (s.type, tuple(s.kd), tuple(s.ks), s.roughness, s.remap) == (11, (0.5,) * 3, (0.5,) * 3, 0, 1)
    assert abs(s.uroughness - 0.1) < 1e-8 and abs(s.vroughness - 0.1) < 1e-8 and s.eta == 0
    g = sm.rough_glass(uroughness=0.2)  # glass.cpp:94-110
    assert (g.type, tuple(g.kr), tuple(g.kt), g.eta, g.vroughness, g.remap, tuple(g.kd)) == (8, (1,) * 3, (1,) * 3, 1.5, 0, 1, (0,) * 3)
    assert len({m.to_bytes() for m in (u, t, s, g)}) == 4


# ---------------- 5. every refusal of the setter's check, with its message ----------------
def test_material_check_refusals_and_messages(sm):
    """bre_check_material_ex is bre_set_materials_ex's check of one record, without a context or a device: every
    refusal of the new types names the material and what is wrong; the accepted records pass."""
    import frosted_refusals

    lib = importlib.import_module("beam-radiance-estimate-pbrt_amd").load_library()
    names = {8: "rough glass", 9: "uber", 10: "translucent", 11: "substrate"}
    buf = ctypes.create_string_buffer(256)
    for m, word in frosted_refusals.bad_records(sm):
        assert lib.bre_check_material_ex(ctypes.byref(m), buf, 256) == 1, word
        msg = buf.value.decode()
        assert word in msg, (word, msg)
        assert "reserved" in msg or names[m.type] in msg, msg  # the message names the material
    for m in frosted_refusals.good_records(sm):
        assert lib.bre_check_material_ex(ctypes.byref(m), buf, 256) == 0 and buf.value == b"", buf.value
    seven = sm.plastic()
    seven.type = 7  # unassigned
    assert lib.bre_check_material_ex(ctypes.byref(seven), buf, 256) == 1 and b"unknown type 7" in buf.value
    t = sm.translucent(reflect=float("nan"))  # the parameter is named as the user wrote it
    assert lib.bre_check_material_ex(ctypes.byref(t), buf, 256) == 1 and b"non-finite reflect (translucent)" in buf.value
    s = sm.substrate()
    s.eta = float("nan")  # a NaN in a field the type does not read is not "non-zero"
    assert lib.bre_check_material_ex(ctypes.byref(s), buf, 256) == 1 and b"non-finite eta, which a substrate" in buf.value
    assert lib.bre_check_material_ex(None, buf, 256) == 1 and lib.bre_check_material_ex(ctypes.byref(sm.uber()), None, 0) == 0


# ---------------- 6. the .pbrt front end ----------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


@pytest.fixture(scope="module")
def pb():
    return importlib.import_module("beam-radiance-estimate-pbrt_amd.pbrt")


def _parse(pb, body, **kw):
    return pb.parse_string(HEAD + body + "WorldEnd\n", **kw)


def test_frosted_fog_parses_to_the_hand_built_scene(pb, sm):
    s = pb.parse_file(os.path.join(ROOT, "scenes", "frosted_fog.pbrt"), materials=True)
    assert s.ok and s.n_errors == 0, s.messages
    case = fs.build("frosted_fog")
    assert s.scene.n_triangles == case.scene.n_triangles == 16
    assert s.scene.to_bytes() == case.scene.to_bytes()
    assert [m.to_bytes() for m in s.materials_ex] == [m.to_bytes() for m in case.materials]
    assert [m.type for m in s.materials_ex] == [sm.MATERIAL_SUBSTRATE, sm.MATERIAL_UBER, sm.MATERIAL_ROUGH_GLASS,
                                                sm.MATERIAL_TRANSLUCENT]
    assert s.triangle_material.tolist() == list(case.tri_mat) == [0] * 2 + [-1] * 2 + [1] * 2 + [-1] * 6 + [2] * 2 + [3] * 2
    assert len(s.lights) == 1 and s.lights[0].to_bytes() == case.lights[0].to_bytes()
    lib = importlib.import_module("beam-radiance-estimate-pbrt_amd").load_library()
    for m in s.materials_ex:  # what the parser writes is what the setter accepts
        assert lib.bre_check_material_ex(ctypes.byref(m), None, 0) == 0


def test_material_statements_with_the_flag(pb, sm):
    """The parser's records byte for byte against the Python helpers: the defaults of the Create...Material
    functions, uber's fallbacks, entries shared by equal materials, remaproughness false, direct and named."""
    s = _parse(pb, 'Material "uber"\n' + FLOOR + 'Material "translucent"\n' + FLOOR + 'Material "substrate"\n' + FLOOR +
               'Material "glass" "float uroughness" [0.2]\n' + FLOOR + 'Material "glass"\n' + FLOOR, materials=True)
    assert s.ok and s.n_errors == 0, s.messages
    assert [m.to_bytes() for m in s.materials_ex] == [
        sm.uber().to_bytes(), sm.translucent().to_bytes(), sm.substrate().to_bytes(),
        sm.rough_glass(uroughness=0.2).to_bytes(), sm.widen(sm.glass()).to_bytes()]  # a direct smooth glass: type 2
    assert s.triangle_material.tolist() == [-1, -1, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    # every parameter, "index" for "eta", uber's u / v given or not, remaproughness false; named and shared
    body = ('MakeNamedMaterial "u" "string type" "uber" "rgb Kd" [0.4 0.3 0.2] "rgb Ks" [0.3 0.4 0.5] "rgb Kr" [0.5 0.5 0.6] '
            '"rgb Kt" [0.7 0.6 0.5] "float roughness" [0.2] "float uroughness" [0.05] "float index" [1.3] '
            '"rgb opacity" [0.6 0.7 0.8] "bool remaproughness" "false"\n'
            'MakeNamedMaterial "t" "string type" "translucent" "rgb Kd" [0.6 0.5 0.4] "rgb Ks" [0.1 0.2 0.3] '
            '"rgb reflect" [0.7 0.7 0.7] "rgb transmit" [0.2 0.3 0.4] "float roughness" [0.3] "bool remaproughness" "false"\n'
            'MakeNamedMaterial "s" "string type" "substrate" "rgb Kd" [0.1 0.2 0.3] "rgb Ks" [0.4 0.5 0.6] '
            '"float uroughness" [0.05] "float vroughness" [0.4] "bool remaproughness" "false"\n'
            'MakeNamedMaterial "g" "string type" "glass" "rgb Kr" [0.9 0.8 0.7] "rgb Kt" [0.6 0.7 0.8] "float eta" [1.33] '
            '"float vroughness" [0.3]\n'
            'NamedMaterial "u"\n' + FLOOR + 'NamedMaterial "t"\n' + FLOOR + 'NamedMaterial "s"\n' + FLOOR +
            'NamedMaterial "g"\n' + FLOOR + 'NamedMaterial "u"\n' + FLOOR +
            'Material "substrate" "rgb Kd" [0.1 0.2 0.3] "rgb Ks" [0.4 0.5 0.6] "float uroughness" [0.05] '
            '"float vroughness" [0.4] "bool remaproughness" "false"\n' + FLOOR)
    s = _parse(pb, body, materials=True)
    assert s.ok and s.n_errors == 0, s.messages
    want = [sm.uber((0.4, 0.3, 0.2), (0.3, 0.4, 0.5), (0.5, 0.5, 0.6), (0.7, 0.6, 0.5), 0.2, 0.05, 0.0, 1.3,
                    (0.6, 0.7, 0.8), False),
            sm.translucent((0.6, 0.5, 0.4), (0.1, 0.2, 0.3), 0.7, (0.2, 0.3, 0.4), 0.3, False),
            sm.substrate((0.1, 0.2, 0.3), (0.4, 0.5, 0.6), 0.05, 0.4, False),
            sm.rough_glass((0.9, 0.8, 0.7), (0.6, 0.7, 0.8), 1.33, 0.0, 0.3, True)]
    assert [m.to_bytes() for m in s.materials_ex] == [m.to_bytes() for m in want]
    assert s.triangle_material.tolist() == [-1, -1, 0, 0, 1, 1, 2, 2, 3, 3, 0, 0, 2, 2]  # equal materials share an entry
    # the flag combines with the others and is refused beyond them
    assert _parse(pb, 'Material "uber"\n' + FLOOR, materials=True, lights=True, media=True).ok
    lib = pb.load_host_library()
    h = ctypes.c_void_p()
    assert lib.bre_pbrt_parse_string_ex(b"WorldBegin WorldEnd", 8, ctypes.byref(h)) == 1


def test_material_refusals_with_the_flag(pb):
    """Texture-valued parameters, "bumpmap", a bad eta and roughnesses that leave no alpha are reported in the
    existing style and the statement falls back to matte."""
    cases = [('Material "uber" "texture Kd" "tex"', 'uber "Kd" must be an rgb or xyz value (textures are not supported)'),
             ('Material "uber" "texture opacity" "tex"', 'uber "opacity" must be an rgb or xyz value'),
             ('Material "uber" "texture roughness" "tex"', 'uber "roughness" must be a float (textures are not supported)'),
             ('Material "translucent" "texture reflect" "tex"', 'translucent "reflect" must be an rgb or xyz value'),
             ('Material "substrate" "texture uroughness" "tex"', 'substrate "uroughness" must be a float'),
             ('Material "glass" "texture vroughness" "tex"', 'glass "vroughness" must be a float'),
             ('Material "glass" "float uroughness" [0.1] "texture bumpmap" "b"', 'glass "bumpmap" is not supported'),
             ('Material "uber" "texture bumpmap" "b"', 'uber "bumpmap" is not supported'),
             ('Material "translucent" "texture bumpmap" "b"', 'translucent "bumpmap" is not supported'),
             ('Material "substrate" "texture bumpmap" "b"', 'substrate "bumpmap" is not supported'),
             ('Material "uber" "float eta" [0]', 'uber "eta" must be finite and > 0'),
             ('Material "glass" "float uroughness" [0.1] "float eta" [-1]', 'glass "eta" must be finite and > 0'),
             ('Material "substrate" "float uroughness" [0] "bool remaproughness" "false"',
              'substrate: the roughnesses must be finite, and > 0 with "remaproughness" false'),
             ('Material "translucent" "float roughness" [-0.1] "bool remaproughness" "false"', 'translucent: the roughnesses'),
             ('Material "glass" "float uroughness" [0.2] "bool remaproughness" "false"', 'glass: the roughnesses')]
    for stmt, word in cases:
        s = _parse(pb, stmt + "\n" + FLOOR, materials=True)
        assert s.n_errors >= 2 and word in s.messages and 'using "matte" in place of this' in s.messages, (stmt, s.messages)
        assert len(s.materials_ex) == 0, stmt  # no table entry: the floor keeps the matte default


def test_default_parse_keeps_its_messages(pb):
    """Without the flag the five pinned messages stand, and the statements fall back as before."""
    body = ('MakeNamedMaterial "g" "string type" "glass" "float uroughness" [0.1]\n'
            'Material "uber" "rgb Kd" [0.1 0.2 0.3]\n' + FLOOR + 'Material "substrate"\n' + FLOOR +
            'Material "translucent"\n' + FLOOR + 'Material "glass"\n' + FLOOR)
    for kw in ({}, {"lights": True}, {"media": True}):
        s = _parse(pb, body, **kw)
        for word in ('glass "uroughness" / "vroughness" must be 0 (rough glass is not supported)',
                     'Material "uber" is not supported (matte, plastic, metal, mirror, named glass); using "matte"',
                     'Material "substrate" is not supported (matte, plastic, metal, mirror, named glass); using "matte"',
                     'Material "translucent" is not supported (matte, plastic, metal, mirror, named glass); using "matte"',
                     'Material "glass" is not supported as a direct statement'):
            assert word in s.messages, (word, s.messages)
        assert len(s.materials_ex) == 0
    d = pb.parse_file(os.path.join(ROOT, "scenes", "frosted_fog.pbrt"))
    assert d.n_errors == 5 and len(d.materials_ex) == 0
