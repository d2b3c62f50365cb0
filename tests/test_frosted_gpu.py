"""Rough glass, uber, translucent and substrate on the GPU (bre_set_materials_ex types 8 .. 11, bre_device_check kind
14) against the pure-Python float32 restatement (tests/refpy_bsdf_full.py, tests/refpy_passes_full.py), bit for bit:
the BSDF of any number of lobes on its own, the two passes on the scenes of tests/frosted_scenes.py.  The whole
iteration, the context walk and the sharded render are held to the project's image bar (relative
L2 <= 1e-5, every pixel above 1e-3 of the maximum within 1e-4).

"Bit for bit" carries the one stated exception of DESIGN.md section 23, the double cos / sin of
TrowbridgeReitzSample11's normal-incidence branch; tests/test_frosted_refpy.py holds every such sample these tests
take outside the margin where it could matter.  Without the feature the setter and the device check refuse type 8
and up, so every test here fails.
"""
import numpy as np
import pytest

import frosted_lobes as fl
import frosted_refs as fr
import frosted_scenes as fs
import refpy_bsdf_full as rf
import refpy_passes_full as rpf
from test_glossy_gpu import BEAM_KEYS, _render_iteration, _sorted, assert_image_bar, bits, rel_l2

pytestmark = pytest.mark.gpu


def same(got, ref):
    """Bit for bit wherever the reference is a number; where the reference itself is a NaN the device's word is a
    NaN too (a NaN's sign and payload are not the arithmetic's: the host and the device differ in them)."""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    nan = np.isnan(ref)
    return bool((bits(got)[~nan] == bits(ref)[~nan]).all() and np.isnan(got[nan]).all())


# ---------------- 1. the BSDF on its own (kind 14) ----------------
def test_lobes_bit_exact(bre):
    x = fl.records()
    assert 50000 <= x.shape[0] < 150000
    ref, stats, _ = fl.reference()
    for k in rf.COUNTERS:
        if not k.startswith(("oren", "lobe_")):  # every lobe, every early return, both halves, the flag sets
            assert stats[k] > 50, (k, stats)
    with bre.BeamGather(0) as g:
        got = g.lobes_check(fl.materials(), x)
    assert np.array_equal(got["type"], ref[:, 7].view(np.int32))
    nans = int(np.isnan(ref).any(axis=1).sum())
    assert 0 < nans < 200  # MicrofacetTransmission::Sample_f at wo.z = 1e-16: the reference's own NaN, kept as one
    assert same(got["wi"], ref[:, :3]) and same(got["pdf"], ref[:, 3]) and same(got["f"], ref[:, 4:7])
    assert same(got["f2"], ref[:, 8:11]) and same(got["pdf2"], ref[:, 11])
    with bre.BeamGather(0) as g:
        # on plastic, metal and matte the BSDF of any number of lobes is the two-lobe one of kind 13
        sel = x[x[:, 8] >= 15]
        old = g.bsdf_check(fl.materials()[15:], np.c_[sel[:, :8], sel[:, 8] - 15])
        new = g.lobes_check(fl.materials(), sel)
        for k in old:
            assert np.array_equal(bits(old[k]), bits(new[k])), k
        # whole records only, of known materials, naming one of them, with a mode and a flag set of 0 or 1
        aux = np.frombuffer(b"".join(m.to_bytes() for m in fl.materials()), np.float32).copy()
        y = np.zeros(24, np.float32)
        r0 = x[0].copy()
        cases = [(r0[:10], aux), (r0, aux[:-1]), (r0, aux[:0]), (np.r_[r0[:8], np.float32(len(fl.materials())), r0[9:]], aux),
                 (np.r_[r0[:8], np.float32(0.5), r0[9:]], aux), (np.r_[r0[:9], np.float32(2), r0[10:]], aux),
                 (np.r_[r0[:10], np.float32(0.5)], aux)]
        for xr, a in cases:
            xr = np.ascontiguousarray(xr, np.float32)
            st = g.lib.bre_device_check(g.h, 14, xr.size, xr.ctypes.data, a.size, a.ctypes.data if a.size else None,
                                        y.ctypes.data)
            assert st == 1, (xr, a.size)


# ---------------- 2. photon pass ----------------
@pytest.mark.parametrize("form", [1, 2, 0], ids=["default", "two-slot", "two-trace"])
@pytest.mark.parametrize("iteration", fs.PHOTON_ITERATIONS)
@pytest.mark.parametrize("name", fs.NAMES)
def test_photon_pass_bit_exact(bre, name, iteration, form):
    case = fs.build(name)
    ref, tags, _, _ = fr.photon_ref(name, iteration)
    # beams born after a transmitting bounce, and (on the scenes with an uber) after a specular uber bounce
    assert ((tags & rf.BSDF_TRANSMISSION) != 0).sum() > 50
    if name in ("uber", "reduced"):
        assert (((tags & rpf.TAG_UBER) != 0) & ((tags & rf.BSDF_SPECULAR) != 0)).sum() > 50
    with bre.BeamGather(0) as g:
        g.set_option(116, form)
        fs.apply(g, case)
        n = g.trace_photons(case.scene, fs.N_PHOTONS, iteration, fs.MAX_DEPTH, fs.RADIUS)
        got = g.get_beams()
        assert n == int(ref["counts"].sum())
        for k in BEAM_KEYS:
            assert np.array_equal(bits(got[k]), bits(ref[k])), k
        if iteration == 0 and form == 1:
            cum = np.cumsum(ref["counts"])
            for k in (1, 2, 3, 5, 17, 64, 65, 127, 200, fs.N_PHOTONS - 1):
                assert g.trace_photons(case.scene, k, 0, fs.MAX_DEPTH, fs.RADIUS) == int(cum[k - 1]), k


@pytest.mark.parametrize("name", fs.DEEP_NAMES)
def test_photon_pass_at_the_deepest_maxdepth(bre, scene_mod_gpu, name):
    """maxdepth 16 (BRE_MAX_DEPTH): the new kernels keep their suspended frames in the block's LDS like the glossy
    ones."""
    case = fs.build(name)
    depth, n = scene_mod_gpu.MAX_DEPTH, fr.DEEP_PHOTONS
    ref, _ = fr.deep_photon_ref(name, depth)
    assert ref["counts"].max() > 8
    with bre.BeamGather(0) as g:
        fs.apply(g, case)
        assert g.trace_photons(case.scene, n, 0, depth, fs.RADIUS) == int(ref["counts"].sum())
        got = g.get_beams()
    for k in BEAM_KEYS:
        assert np.array_equal(bits(got[k]), bits(ref[k])), k


# ---------------- 3. camera pass ----------------
def _camera(bre, case, iteration):
    import torch

    surf = torch.zeros((fs.CAM_W * fs.CAM_H, 3), dtype=torch.float32, device="cuda")
    with bre.BeamGather(0) as g:
        fs.apply(g, case)
        n = g.camera_pass(case.scene, fs.CAM_W, fs.CAM_H, iteration, fs.CAM_DEPTH, surface=surf)
        seg = g.get_segments()
    torch.cuda.synchronize()
    return n, seg, surf.cpu().numpy()


@pytest.mark.parametrize("iteration", fs.CAMERA_ITERATIONS)
@pytest.mark.parametrize("name", fs.NAMES)
def test_camera_pass_bit_exact(bre, name, iteration):
    """Segments and surface radiance, bit for bit: specularBounce per sampled lobe, EstimateDirect under
    BSDF_ALL & ~BSDF_SPECULAR on both sides of the surface."""
    ref, info, _, _ = fr.camera_ref(name, iteration)
    assert len(info["lit_through"]) >= 20  # pixels lit through a transmissive surface
    if name == "uber" and iteration == 0:
        assert info["le_after_uber_specular"]  # pixels that carry Le after a specular bounce on an uber
    n, gpu, surf = _camera(bre, fs.build(name), iteration)
    assert n == gpu["o"].shape[0] == ref["o"].shape[0]
    a, r = _sorted(gpu), _sorted(ref)
    assert np.array_equal(a["pixel"], r["pixel"]) and np.array_equal(a["depth"], r["depth"])
    for k in ("o", "p", "d", "tmax"):
        assert np.array_equal(bits(a[k]), bits(r[k])), k
    assert np.array_equal(bits(surf), bits(ref["surface"]))


# ---------------- 4. an uber with Kd alone is the matte wall ----------------
def test_uber_kd_alone_equals_matte_context(bre):
    a, b = fs.build("uber_kd"), fs.build("uber_kd_plain")
    assert a.materials and not b.materials
    beams = []
    for case in (a, b):
        with bre.BeamGather(0) as g:
            fs.apply(g, case)
            g.trace_photons(case.scene, fs.N_PHOTONS, 0, fs.MAX_DEPTH, fs.RADIUS)
            beams.append(g.get_beams())
    assert beams[0]["radius"].shape[0] > fs.N_PHOTONS
    for k in BEAM_KEYS:
        assert np.array_equal(bits(beams[0][k]), bits(beams[1][k])), k
    (na, sa, fa), (nb, sb, fb) = _camera(bre, a, 0), _camera(bre, b, 0)
    assert na == nb > 0 and fa.max() > 0
    for k in ("o", "p", "d", "tmax", "pixel", "depth"):
        assert np.array_equal(sa[k].view(np.uint32), sb[k].view(np.uint32)), k
    assert np.array_equal(bits(fa), bits(fb))


# ---------------- 5. whole iteration ----------------
@pytest.mark.parametrize("name", ["slab", "uber"])
def test_render_iteration(bre, oracle, scene_mod_gpu, name):
    case = fs.build(name)
    R = 0.05
    p = scene_mod_gpu.render_params(fs.CAM_W, fs.CAM_H, iterations=1, photons=fs.N_PHOTONS, max_depth=5, radius=R,
                                    alpha=0.5)
    beams, _ = rpf.trace_photons(fr.scene(name), fs.N_PHOTONS, 0, 5, R)
    cam = fr.camera_ref(name, 0)[0]
    bf = oracle.bruteforce(beams, cam, R)
    ref = cam["surface"].astype(np.float64)
    np.add.at(ref, cam["pixel"], bf["seg_rgb_exact"])
    with bre.BeamGather(0) as g:
        fs.apply(g, case)
        got = _render_iteration(g, case.scene, p)
    print(f"{name} {fs.CAM_W}x{fs.CAM_H} iteration: rel-L2 {rel_l2(got, ref):.3e}")
    assert ref.max() > 0
    assert_image_bar(got, ref)


# ---------------- 6. context walk ----------------
def test_context_walk_lobed_and_narrow_tables(bre, scene_mod_gpu):
    """A rough-glass table swapped for a narrow glass table and back on one context: each render is what a fresh
    context gives."""
    sm = scene_mod_gpu
    case = fs.build("slab")
    k_glass = [k for k, m in enumerate(case.materials) if m.type == sm.MATERIAL_ROUGH_GLASS][0]
    tri_glass = [0 if k == k_glass else -1 for k in case.tri_mat]  # the box alone, as smooth glass in a narrow table
    p = sm.render_params(24, 24, iterations=1, photons=fs.N_PHOTONS, max_depth=5, radius=0.05, alpha=0.5)
    smooth = [sm.glass(1.0, 1.0, 1.5)]

    def fresh(mats, tri_mat):
        with bre.BeamGather(0) as g:
            g.set_lights(case.lights)
            g.set_materials(mats, tri_mat)
            return _render_iteration(g, case.scene, p)

    matte, rough, clear = fresh([], []), fresh(case.materials, case.tri_mat), fresh(smooth, tri_glass)
    assert matte.max() > 0 and rel_l2(rough, matte) > 1e-3 and rel_l2(clear, rough) > 1e-3
    with bre.BeamGather(0) as g:
        g.set_lights(case.lights)
        g.set_materials(case.materials, case.tri_mat)
        assert_image_bar(_render_iteration(g, case.scene, p), rough, l2=1e-6)
        g.set_materials(smooth, tri_glass)
        assert_image_bar(_render_iteration(g, case.scene, p), clear, l2=1e-6)
        g.set_materials(case.materials, case.tri_mat)
        assert_image_bar(_render_iteration(g, case.scene, p), rough, l2=1e-6)
        g.set_materials()
        assert_image_bar(_render_iteration(g, case.scene, p), matte, l2=1e-6)
        with pytest.raises(bre.BreError) as e:  # a refused table leaves the context as it was
            g.set_materials([sm.rough_glass(1, 1, 1.5, 0.0, 0.0)], [0] * case.scene.n_triangles)
        assert e.value.status == 1 and "BRE_MATERIAL_GLASS" in str(e.value)
        assert_image_bar(_render_iteration(g, case.scene, p), matte, l2=1e-6)


# ---------------- 7. sharded ----------------
@pytest.mark.parametrize("shards", [1, 2])
def test_render_sharded_with_lobed_table(bre, scene_mod_gpu, shards):
    case = fs.build("sheet")
    p = scene_mod_gpu.render_params(24, 24, iterations=2, photons=fs.N_PHOTONS, max_depth=5, radius=0.05, alpha=0.5)
    with bre.BeamGather(0) as g:
        fs.apply(g, case)
        whole = g.render(case.scene, p)
    ctxs = [bre.BeamGather(0) for _ in range(shards)]
    try:
        for c in ctxs[:-1]:
            fs.apply(c, case)
        if shards > 1:
            ctxs[-1].set_lights(case.lights)
            with pytest.raises(bre.BreError) as e:
                bre.render_sharded(ctxs, case.scene, p)
            assert e.value.status == 1 and "materials" in str(e.value)
        fs.apply(ctxs[-1], case)
        img = bre.render_sharded(ctxs, case.scene, p)
    finally:
        for c in ctxs:
            c.close()
    assert whole.max() > 0 and rel_l2(img, whole) <= 1e-6


# ---------------- 8. the setter's refusals for the new types ----------------
def test_set_materials_ex_refusals_of_the_new_types(bre, scene_mod_gpu):
    import frosted_refusals

    sm = scene_mod_gpu
    case = fs.build("slab")
    n = case.scene.n_triangles
    with bre.BeamGather(0) as g:
        fs.apply(g, case)
        before = g.trace_photons(case.scene, 500, 0, 5, 0.05)
        for m, word in frosted_refusals.bad_records(sm):
            with pytest.raises(bre.BreError) as e:
                g.set_materials([m], [0] * n)
            assert e.value.status == 1 and "material 0" in str(e.value) and word in str(e.value), (word, str(e.value))
        assert g.trace_photons(case.scene, 500, 0, 5, 0.05) == before  # the context keeps what it held
        for m in frosted_refusals.good_records(sm):
            g.set_materials([m], [0] * n)
        assert g.trace_photons(case.scene, 500, 0, 5, 0.05) > 0


# ---------------- 9. .pbrt ----------------
def test_pbrt_frosted_fog_equals_library_render(bre):
    """bre_pbrt --materials' path on scenes/frosted_fog.pbrt at 64 x 48, 3 iterations, 20k photons: the library render
    of the hand-built scene (the parse itself is held to it byte for byte in tests/test_frosted_refpy.py)."""
    import importlib
    import os

    pb = importlib.import_module("beam-radiance-estimate-pbrt_amd.pbrt")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "scenes", "frosted_fog.pbrt")).read()
    text = (text.replace("[256]", "[64]", 1).replace("[256]", "[48]", 1).replace("[50000]", "[20000]")
            .replace('"integer iterations" [32]', '"integer iterations" [3]')
            .replace('"float initialbeamradius" [0.01]', '"float initialbeamradius" [0.05]'))
    s = pb.parse_string(text, materials=True)
    assert s.ok and s.n_errors == 0 and len(s.lights) == 1 and len(s.materials_ex) == 4, s.messages
    assert (s.params.width, s.params.height, s.params.iterations, s.params.photons_per_iteration) == (64, 48, 3, 20000)
    img = s.render(write_files=False)
    case = fs.build("frosted_fog")
    with bre.BeamGather(0) as g:
        fs.apply(g, case)
        L = g.render(case.scene, s.params)
        g.set_materials()
        L_matte = g.render(case.scene, s.params)
    ref = pb.film_finalize(L.reshape(-1, 3), s.film["scale"]).reshape(L.shape)
    assert img.shape == (48, 64, 3) and img.max() > 0
    assert rel_l2(L, L_matte) > 1e-3  # the file's materials reached the render
    assert_image_bar(img, ref)
    assert rel_l2(s.render(devices=[0, 0], write_files=False), img) <= 1e-6  # two contexts: the table is set on both
