"""Mix materials without a GPU: the restatement (tests/refpy_mix.py, tests/refpy_passes_mix.py) held to answers
derived by hand from the reference text, the coverage of the inputs the GPU tests use, and the records and refusals of
the C ABI (bre_check_material_ex, bre_check_material_table_ex: no context, no device).

1. The restatement: a mix of a matte with itself, amount 1 against a mirror, two specular lobes, a nest's order of
   multiplication, EstimateDirect's flag set.
2. Every counter a mix brings is reached by the scenes of tests/mix_scenes.py and by the records of tests/mix_lobes.py.
3. scene.mix's bytes, the layout through ctypes, every refusal with its message.
Without the feature scene.mix does not exist and the library refuses type 12 as unknown: every test here fails.
"""
import ctypes
import importlib
import math
import os

import numpy as np
import pytest

import mix_lobes as ml
import mix_refs as mr
import mix_scenes as ms
import refpy_bsdf as rb
import refpy_bsdf_full as rf
import refpy_mix as rm
import refpy_passes_mix as rpm
from refpy_photon import INV_PI, f32

Q = rb.FRAME


@pytest.fixture(scope="module")
def sm():
    return importlib.import_module("beam-radiance-estimate-pbrt_amd.scene")


def _n3(v):
    v = np.asarray(v, np.float64)
    return tuple(f32(x) for x in v / np.linalg.norm(v))


def _bits(v):
    return np.asarray(v, np.float32).view(np.uint32).tolist()


# ---------------- 1. the restatement, by hand ----------------
def test_mix_of_a_matte_with_itself(sm):
    """2 components; f = t * (kd / pi) + (1 - t) * (kd / pi) in that float order; Pdf is exactly the matte's."""
    kd, t = (f32(0.6), f32(0.5), f32(0.4)), f32(0.3)
    table = [sm.matte(kd), sm.mix(0, 0, float(t))]
    b, matte = rm.bsdf_of(table, 1), rf.bsdf_of(table[0])
    assert len(b.lobes) == 2 and len(b.matching(rf.BSDF_NON_SPECULAR)) == 2
    wo, wi = _n3((0.3, 0.2, 0.93)), _n3((-0.5, 0.1, 0.4))
    want = tuple(f32(f32(t * f32(k * INV_PI)) + f32(f32(f32(1) - t) * f32(k * INV_PI))) for k in kd)
    assert _bits(b.f(Q, wo, wi)) == _bits(want)
    assert _bits(b.pdf(Q, wo, wi)) == _bits(matte.pdf(Q, wo, wi))
    s = b.sample(Q, wo, 0.7, 0.4)
    m = matte.sample(Q, wo, f32(f32(f32(0.7) * f32(2)) - f32(1)), 0.4)  # the second component, u0 remapped
    assert _bits(s[0]) == _bits(m[0]) and _bits(s[1]) == _bits(m[1]) and _bits(s[2]) == _bits(want)


def test_amount_1_is_not_the_first_material(sm):
    """mix(matte, mirror, amount 1): the mirror's lobe is there with a black scale, takes half of the samples and
    returns the mirror direction with pdf exactly 0.5 and f = 0; in the photon walk that ends the path."""
    table = [sm.matte((0.6, 0.5, 0.4)), sm.widen(sm.mirror(0.9)), sm.mix(0, 1, 1.0)]
    b = rm.bsdf_of(table, 2)
    assert len(b.lobes) == 2 and b.lobes[1].zero_scale() and not b.lobes[0].zero_scale()
    wo = _n3((0.3, 0.2, 0.93))
    wi, pdf, f, typ = b.sample(Q, wo, 0.5, 0.25)
    assert _bits(wi) == _bits((-wo[0], -wo[1], wo[2])) and pdf == f32(0.5) and f == (0, 0, 0)
    assert typ == rf.BSDF_SPECULAR | rf.BSDF_REFLECTION
    first = b.sample(Q, wo, 0.25, 0.25)  # the matte lobe: its pdf is halved too, the mirror's Pdf adding 0
    plain = rf.bsdf_of(table[0]).sample(Q, wo, 0.5, 0.25)
    assert _bits(first[0]) == _bits(plain[0]) and _bits(first[1]) == _bits(f32(plain[1] / f32(2)))
    # The same photons onto the floor of `polished` in vacuum, as the plain matte and as the mix.  Up to the floor's
    # Get2D both walks draw the same numbers; a photon whose u0 picks the black lobe ends there with its one beam,
    # where the matte's goes on with probability lum(kd): over those photons the beam count is below the matte's.
    # Over the whole pass it is not: the photons that pick the matte lobe carry f / (pdf / 2), twice the matte's
    # weight, and never fall to the roulette (400 photons of `polished` in fog: 1134 beams against the matte's 1096).
    meshes, table, _, lights, _, _ = ms.meshes_of("polished")
    plain = [m[:4] + (None,) + tuple(m[5:]) for m in meshes]
    tri_mix = sum(([-1 if m[4] is None else 2] * (len(m[1]) // 3) for m in meshes), [])
    tri_matte = [0 if k >= 0 else -1 for k in tri_mix]
    scene = sm.make_scene(plain)
    mix_sc = rpm.Scene(scene, lights, [table[1], table[0], sm.mix(0, 1, 1.0)], tri_mix)
    matte_sc = rpm.Scene(scene, lights, [table[1]], tri_matte)
    a = rpm.trace_photons(mix_sc, 400, 0, 5, 0.01)[0]
    b2 = rpm.trace_photons(matte_sc, 400, 0, 5, 0.01)[0]
    ca, cb = a["counts"], b2["counts"]
    fa, fb = np.cumsum(ca) - ca, np.cumsum(cb) - cb  # each photon's first beam
    live = (ca > 0) & (cb > 0)
    assert live.sum() > 300 and np.array_equal(live, (ca > 0) | (cb > 0))
    assert np.array_equal(a["end"][fa[live]].view(np.uint32), b2["end"][fb[live]].view(np.uint32))
    floor = np.zeros(400, bool)
    floor[live] = a["end"][fa[live]][:, 1] < 1e-6
    ended = floor & (ca == 1)
    # half of the samples go to the black lobe (over 200 photons the share's standard deviation is 0.035)
    assert floor.sum() >= 200 and 0.4 < ended.sum() / floor.sum() < 0.6
    assert ca[ended].sum() < cb[ended].sum()


def test_two_specular_lobes(sm):
    """mix(mirror, glass): no pdf sum and no f re-evaluation; pdf = the lobe's / 2; the sampled type is the one
    FresnelSpecular sets."""
    table = [sm.widen(sm.mirror(0.9)), sm.widen(sm.glass(0.8, 0.9, 1.5)), sm.mix(0, 1, 0.25)]
    b = rm.bsdf_of(table, 2)
    assert [x.type & rf.BSDF_SPECULAR for x in b.lobes] == [16, 16] and not b.matching(rf.BSDF_NON_SPECULAR)
    wo = _n3((0.3, 0.2, 0.93))
    wi, pdf, f, typ = b.sample(Q, wo, 0.2, 0.5, mode=rf.IMPORTANCE)
    ac = f32(abs(wo[2]))
    assert pdf == f32(0.5) and typ == rf.BSDF_SPECULAR | rf.BSDF_REFLECTION
    assert _bits(f) == _bits(tuple(f32(f32(0.25) * f32(f32(f32(1) * f32(0.9)) / ac)) for _ in range(3)))
    F, _ = rm.fr_dielectric(wo[2], f32(1), f32(1.5))
    u_reflect, u_transmit = f32(0.5) + F / 4, f32(0.5) + F / 2 + f32(0.2)  # remapped below and above F
    r = b.sample(Q, wo, u_reflect, 0.5, mode=rf.IMPORTANCE)
    t = b.sample(Q, wo, u_transmit, 0.5, mode=rf.IMPORTANCE)
    assert r[3] == rf.BSDF_SPECULAR | rf.BSDF_REFLECTION and _bits(r[1]) == _bits(f32(F / f32(2)))
    assert t[3] == rf.BSDF_SPECULAR | rf.BSDF_TRANSMISSION and _bits(t[1]) == _bits(f32(f32(f32(1) - F) / f32(2)))
    assert t[0][2] < 0 < r[0][2]
    assert b.f(Q, wo, r[0]) == (0, 0, 0) and b.pdf(Q, wo, r[0]) == 0


def test_a_nest_multiplies_outermost_last(sm):
    """s_out * (s_in * f) in bits, which (s_out * s_in) * f is not on a chosen input."""
    s_in, s_out = f32(0.7), f32(0.3)
    table = [sm.matte((0.6, 0.5, 0.4)), sm.mix(0, 0, float(s_in)), sm.mix(1, 1, float(s_out))]
    b = rm.bsdf_of(table, 2)
    assert len(b.lobes) == 4 and all(x.depth == 2 for x in b.lobes)
    wo, wi = _n3((0.3, 0.2, 0.93)), _n3((-0.5, 0.1, 0.4))
    lobe = b.lobes[0]  # the first matte lobe under s_in, then under s_out
    f = tuple(f32(k * INV_PI) for k in (f32(0.6), f32(0.5), f32(0.4)))
    nested = tuple(f32(s_out * f32(s_in * x)) for x in f)
    folded = tuple(f32(f32(s_out * s_in) * x) for x in f)
    assert _bits(lobe.f(wo, wi, rf.RADIANCE)) == _bits(nested)
    assert _bits(nested) != _bits(folded)  # the input tells the two orders apart


def test_estimate_direct_sees_one_lobe_of_two(sm):
    """BSDF_ALL & ~BSDF_SPECULAR on mix(glass, matte) matches the matte's lobe alone: Pdf and Sample_f over one
    component, f its scaled value."""
    t = f32(0.25)
    table = [sm.widen(sm.glass(1.0, 1.0, 1.5)), sm.matte((0.6, 0.5, 0.4)), sm.mix(0, 1, float(t))]
    b, matte = rm.bsdf_of(table, 2), rf.bsdf_of(table[1])
    assert len(b.matching(rf.BSDF_ALL)) == 2 and len(b.matching(rf.BSDF_NON_SPECULAR)) == 1
    wo, wi = _n3((0.3, 0.2, 0.93)), _n3((-0.5, 0.1, 0.4))
    s2 = f32(f32(1) - t)
    want = tuple(f32(s2 * f32(k * INV_PI)) for k in (f32(0.6), f32(0.5), f32(0.4)))
    assert _bits(b.f(Q, wo, wi, rf.BSDF_NON_SPECULAR)) == _bits(want)
    assert _bits(b.pdf(Q, wo, wi, rf.BSDF_NON_SPECULAR)) == _bits(matte.pdf(Q, wo, wi))
    s, m = b.sample(Q, wo, 0.7, 0.4, rf.BSDF_NON_SPECULAR), matte.sample(Q, wo, 0.7, 0.4)
    assert _bits(s[0]) == _bits(m[0]) and _bits(s[1]) == _bits(m[1]) and _bits(s[2]) == _bits(want)
    assert _bits(b.pdf(Q, wo, wi)) == _bits(f32(matte.pdf(Q, wo, wi) / f32(2)))  # BSDF_ALL: two components


# ---------------- 2. coverage of the inputs the GPU tests use ----------------
def test_every_counter_is_reached_by_the_scenes():
    total = {k: 0 for k in rm.MIX_COUNTERS}
    for name in ms.NAMES:
        for it in ms.CAMERA_ITERATIONS:
            stats = [mr.camera_ref(name, it)[2]] + ([mr.photon_ref(name, it)[2]] if name in ms.PHOTON_NAMES else [])
            for st in stats:
                for k in total:
                    total[k] += st[k]
    print(total)
    for k, v in total.items():
        assert v >= 20, (k, total)


def test_every_counter_is_reached_by_the_lobe_records():
    stats = ml.total_stats()
    print({k: stats[k] for k in rm.MIX_COUNTERS})
    for k in rm.MIX_COUNTERS:
        assert stats[k] >= 50, (k, stats)
    assert 20000 <= sum(ml.records(t).shape[0] for t in range(len(ml.tables()))) <= 80000


# ---------------- 3. records and refusals ----------------
def test_mix_record_bytes_and_layout(sm):
    assert ctypes.sizeof(sm.MaterialEx) == 112 and sm.MaterialEx.kd.offset == 32 and sm.MaterialEx.reserved.offset == 100
    assert (sm.MATERIAL_MIX, sm.MAX_MIX_DEPTH, sm.MAX_BXDFS) == (12, 4, 8)
    m = sm.mix(3, 5)  # CreateMixMaterial's default amount, mixmat.cpp:69-70
    assert (m.type, tuple(m.amount), tuple(m.mix_child), tuple(m.reserved)) == (12, (0.5,) * 3, (3, 5), (3, 5, 0))
    words = np.frombuffer(m.to_bytes(), np.int32)
    want = np.zeros(28, np.int32)
    want[0] = 12
    want[8:11] = np.array([0.5] * 3, np.float32).view(np.int32)  # amount in kd's words
    want[25], want[26] = 3, 5                                    # the children in reserved[0..1]
    assert words.tolist() == want.tolist()
    m.amount = sm.F3(0.25, 0.5, 0.75)
    m.mix_child[1] = 4
    assert tuple(m.kd) == (0.25, 0.5, 0.75) and tuple(m.reserved) == (3, 4, 0)
    assert tuple(sm.mix(0, 1, (0.1, 0.2, 0.3)).amount) == tuple(sm.F3(0.1, 0.2, 0.3))


def test_refusals_and_messages(sm):
    import mix_refusals

    bre = importlib.import_module("beam-radiance-estimate-pbrt_amd")
    lib = bre.load_library()
    assert "bre_check_material_table_ex" in bre.EXPORTS
    buf = ctypes.create_string_buffer(512)
    for m, word in mix_refusals.bad_records(sm):
        assert lib.bre_check_material_ex(ctypes.byref(m), buf, 512) == 1, word
        assert word in buf.value.decode() and "mix" in buf.value.decode(), (word, buf.value)
    assert lib.bre_check_material_ex(ctypes.byref(sm.mix(0, 0)), buf, 512) == 0 and buf.value == b""
    for table, word in mix_refusals.bad_tables(sm):
        arr = (sm.MaterialEx * len(table))(*table)
        assert lib.bre_check_material_table_ex(arr, len(table), buf, 512) == 1, word
        assert word in buf.value.decode(), (word, buf.value)
        assert word in bre.BeamGather.check_material_table(table)
    for table in mix_refusals.good_tables(sm):
        assert bre.BeamGather.check_material_table(table) == "", table
    for t in range(len(ml.tables())):
        assert bre.BeamGather.check_material_table(ml.tables()[t]) == ""
    for name in ms.NAMES + ("mix_fog",):
        assert bre.BeamGather.check_material_table(ms.build(name).materials) == "", name
    # a child without a BSDF: without media the interface's own record is refused first
    msg = bre.BeamGather.check_material_table([sm.widen(sm.interface()), sm.matte(0.5), sm.mix(0, 1)])
    assert "material 0 has unknown type 3 (BRE_MATERIAL_INTERFACE" in msg
    # records of every other type still have all three reserved words 0, in the words they had
    other = sm.matte(0.5)
    other.reserved[0] = 1
    assert lib.bre_check_material_ex(ctypes.byref(other), buf, 512) == 1 and buf.value == b"non-zero reserved words"
    assert bre.BeamGather.check_material_table([other]) == "material 0 has non-zero reserved words"
    # amount is clamped like every colour of the ABI: beyond [0, 1] is accepted
    assert lib.bre_check_material_table_ex(None, 0, buf, 512) == 1
    assert math.isclose(sm.mix(0, 0, 2.0).amount[0], 2.0)


# ---------------- 4. the .pbrt front end: the subsurface materials ----------------
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


def test_subsurface_materials_with_the_flag(pb, sm):
    """subsurface and kdsubsurface are their dielectric boundary (photonbeam.cpp never reads isect.bssrdf): a glass
    where both roughnesses are 0, else a rough glass, with Kr = Kt = 1, eta 1.33, remaproughness true; one warning a
    statement; what only the BSSRDF reads is accepted and ignored."""
    body = ('Material "subsurface"\n' + FLOOR +
            'Material "kdsubsurface" "rgb Kd" [0.5 0.4 0.3] "rgb mfp" [1 2 3] "float uroughness" [0.2]\n' + FLOOR +
            'MakeNamedMaterial "skin" "string type" "subsurface" "string name" "Skin1" "rgb sigma_a" [0.1 0.2 0.3] '
            '"rgb sigma_s" [1 2 3] "float scale" [2] "float g" [0.5] "float eta" [1.4] "rgb Kr" [0.9 0.8 0.7] '
            '"rgb Kt" [0.6 0.7 0.8] "float uroughness" [0.1] "float vroughness" [0.3] "bool remaproughness" "false"\n'
            'NamedMaterial "skin"\n' + FLOOR + 'Material "kdsubsurface"\n' + FLOOR)
    s = _parse(pb, body, materials=True)
    assert s.ok and s.n_errors == 0, s.messages
    want = [sm.widen(sm.glass(1.0, 1.0, 1.33)), sm.rough_glass(1.0, 1.0, 1.33, 0.2, 0.0, True),
            sm.rough_glass((0.9, 0.8, 0.7), (0.6, 0.7, 0.8), 1.4, 0.1, 0.3, False)]
    assert [m.to_bytes() for m in s.materials_ex] == [m.to_bytes() for m in want]
    assert s.triangle_material.tolist() == [-1, -1, 0, 0, 1, 1, 2, 2, 0, 0]  # the two smooth defaults share an entry
    assert s.messages.count("the photon-beam integrator never reads the BSSRDF") == 4  # one warning a statement
    assert 'Material "subsurface"' in s.messages and 'Material "kdsubsurface"' in s.messages
    assert "rough glass of eta 1.4" in s.messages and "a glass of eta 1.33" in s.messages
    for stmt, word in (('Material "subsurface" "texture sigma_a" "t"', 'subsurface "sigma_a" must be an rgb or xyz value'),
                       ('Material "kdsubsurface" "texture mfp" "t"', 'kdsubsurface "mfp" must be an rgb or xyz value'),
                       ('Material "subsurface" "texture bumpmap" "b"', 'subsurface "bumpmap" is not supported'),
                       ('Material "kdsubsurface" "float eta" [0]', 'kdsubsurface "eta" must be finite and > 0')):
        bad = _parse(pb, stmt + "\n" + FLOOR, materials=True)
        assert word in bad.messages and 'using "matte" in place of this' in bad.messages, (stmt, bad.messages)
        assert len(bad.materials_ex) == 0, stmt


def test_default_parse_keeps_its_messages(pb):
    body = 'Material "mix"\n' + FLOOR + 'Material "subsurface"\n' + FLOOR + 'Material "kdsubsurface"\n' + FLOOR
    for kw in ({}, {"lights": True}, {"media": True}):
        s = _parse(pb, body, **kw)
        for name in ("mix", "subsurface", "kdsubsurface"):
            word = 'Material "%s" is not supported (matte, plastic, metal, mirror, named glass); using "matte"' % name
            assert word in s.messages, (word, s.messages)
        assert len(s.materials_ex) == 0 and "BSSRDF" not in s.messages


# ---------------- 5. the .pbrt front end: mix ----------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMED = ('MakeNamedMaterial "m" "string type" "mirror"\n'
         'MakeNamedMaterial "d" "string type" "matte" "rgb Kd" [0.6 0.5 0.4]\n'
         'MakeNamedMaterial "g" "string type" "glass" "float eta" [1.33]\n'
         'MakeNamedMaterial "p" "string type" "plastic"\n')


def test_mix_fog_parses_to_the_hand_built_scene(pb, sm):
    bre = importlib.import_module("beam-radiance-estimate-pbrt_amd")
    s = pb.parse_file(os.path.join(ROOT, "scenes", "mix_fog.pbrt"), materials=True)
    assert s.ok and s.n_errors == 0, s.messages
    case = ms.build("mix_fog")
    assert s.scene.n_triangles == case.scene.n_triangles == 14
    assert s.scene.to_bytes() == case.scene.to_bytes()
    assert [m.to_bytes() for m in s.materials_ex] == [m.to_bytes() for m in case.materials]
    assert [m.type for m in s.materials_ex] == [1, 4, 12, 5, 6, 12, 11, 12, 2, 4, 12]
    assert s.triangle_material.tolist() == list(case.tri_mat) == [2] * 2 + [-1] * 2 + [7] * 2 + [-1] * 6 + [10] * 2
    assert len(s.lights) == 1 and s.lights[0].to_bytes() == case.lights[0].to_bytes()
    assert bre.BeamGather.check_material_table(s.materials_ex) == ""  # what the parser writes the setter accepts


def test_mix_statements_with_the_flag(pb, sm):
    """The parser's records byte for byte against the Python helpers: direct and named, the default amount, rgb and
    float amounts, an undeclared child as a matte of the statement's own parameters, shared entries, a nest."""
    W = sm.widen
    body = (NAMED +
            'Material "mix" "string namedmaterial1" "m" "string namedmaterial2" "d"\n' + FLOOR +           # direct, default
            'MakeNamedMaterial "x" "string type" "mix" "string namedmaterial1" "g" "string namedmaterial2" "d" '
            '"rgb amount" [0.2 0.5 0.8]\n'
            'NamedMaterial "x"\n' + FLOOR +                                                                # named, rgb
            'Material "mix" "string namedmaterial1" "d" "string namedmaterial2" "nope" "float amount" [0.25] '
            '"rgb Kd" [0.1 0.2 0.3]\n' + FLOOR +                                                           # undeclared
            'MakeNamedMaterial "y" "string type" "mix" "string namedmaterial1" "x" "string namedmaterial2" "p" '
            '"float amount" [0.75]\n'
            'NamedMaterial "y"\n' + FLOOR +                                                                # a nest
            'Material "mix" "string namedmaterial1" "m" "string namedmaterial2" "d"\n' + FLOOR)            # shared
    s = _parse(pb, body, materials=True)
    assert s.n_errors == 1 and 'Named material "nope" undefined.  Using "matte"' in s.messages, s.messages
    want = [W(sm.mirror(0.9)), sm.matte((0.6, 0.5, 0.4)), sm.mix(0, 1), W(sm.glass(1.0, 1.0, 1.33)),
            sm.mix(3, 1, (0.2, 0.5, 0.8)), sm.matte((0.1, 0.2, 0.3)), sm.mix(1, 5, 0.25), sm.plastic(), sm.mix(4, 7, 0.75)]
    assert [m.to_bytes() for m in s.materials_ex] == [m.to_bytes() for m in want]
    assert s.triangle_material.tolist() == [-1, -1, 2, 2, 4, 4, 6, 6, 8, 8, 2, 2]
    # a texture-valued amount is reported and falls back to 0.5
    t = _parse(pb, NAMED + 'Material "mix" "string namedmaterial1" "m" "string namedmaterial2" "d" "texture amount" "t"\n' +
               FLOOR, materials=True)
    assert 'mix "amount" must be an rgb or xyz value (textures are not supported); using 0.5' in t.messages
    assert [m.to_bytes() for m in t.materials_ex] == [m.to_bytes() for m in want[:3]]
    # a table-level refusal is reported at the statement with the library's message; the statement falls back to matte
    deep = NAMED + "".join('MakeNamedMaterial "n%d" "string type" "mix" "string namedmaterial1" "%s" '
                           '"string namedmaterial2" "d"\n' % (k, "n%d" % (k - 1) if k else "d") for k in range(5))
    r = _parse(pb, deep + 'NamedMaterial "n4"\n' + FLOOR + 'NamedMaterial "n3"\n' + FLOOR, materials=True)
    assert "mix: material 5 has a nest 5 mixes deep (at most BRE_MAX_MIX_DEPTH = 4); using \"matte\"" in r.messages, r.messages
    assert r.triangle_material.tolist() == [-1, -1, -1, -1, 4, 4] and len(r.materials_ex) == 5  # n3 is four deep
