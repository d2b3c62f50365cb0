"""Plastic, metal and Oren-Nayar on the GPU (bre_set_materials_ex, bre_device_check kind 13) against the pure-Python
float32 restatement (tests/refpy_bsdf.py, tests/refpy_passes_bsdf.py), bit for bit: the BSDF on its own, the two
passes on the scenes of tests/glossy_scenes.py.  The whole iteration, the context walk and the sharded render are
held to the project's image bar (relative L2 <= 1e-5, every pixel above 1e-3 of the maximum
within 1e-4).

"Bit for bit" carries the one stated exception of DESIGN.md section 23: the double cos / sin of
TrowbridgeReitzSample11's normal-incidence branch.  tests/test_glossy_refpy.py checks that none of the samples
these tests take lies within the margin where the device's pair (relative error <= 2^-50) could round differently
from the host libm.

The restatement is the slow side: tests/glossy_refs.py and tests/glossy_lobes.py compute each reference once.
"""
import numpy as np
import pytest

import glossy_lobes as gl
import glossy_refs as gr
import glossy_scenes as gs
import refpy_passes_bsdf as rpb
import specular_scenes

pytestmark = pytest.mark.gpu

BEAM_KEYS = ("start", "end", "radius", "power")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def assert_image_bar(got, ref, l2=1e-5):
    """relative L2 <= 1e-5, every pixel above 1e-3 of the maximum within 1e-4."""
    got, ref = np.asarray(got, np.float64).reshape(-1, 3), np.asarray(ref, np.float64).reshape(-1, 3)
    assert rel_l2(got, ref) <= l2, rel_l2(got, ref)
    bright = ref.max(axis=1) > 1e-3 * ref.max()
    assert (np.abs(got - ref)[bright] <= 1e-4 * np.abs(ref[bright]).max(axis=1, keepdims=True)).all()


# ---------------- 1. the BSDF on its own (kind 13) ----------------
def test_bsdf_bit_exact(bre):
    x = gl.records()
    assert 40000 <= x.shape[0] <= 60000
    ref, stats, _ = gl.reference()
    for k, v in stats.items():
        assert v > 50, (k, stats)
    with bre.BeamGather(0) as g:
        got = g.bsdf_check(gl.materials(), x)
    assert np.array_equal(got["type"], ref[:, 7].view(np.int32))
    assert np.array_equal(bits(got["wi"]), bits(ref[:, :3]))
    assert np.array_equal(bits(got["pdf"]), bits(ref[:, 3]))
    assert np.array_equal(bits(got["f"]), bits(ref[:, 4:7]))
    assert np.array_equal(bits(got["f2"]), bits(ref[:, 8:11]))
    assert np.array_equal(bits(got["pdf2"]), bits(ref[:, 11]))
    with bre.BeamGather(0) as g:  # whole records only, of known materials, naming one of them
        aux = np.frombuffer(b"".join(m.to_bytes() for m in gl.materials()), np.float32).copy()
        y = np.zeros(24, np.float32)
        cases = [(x[:1].ravel()[:8], aux), (x[:1].ravel(), aux[:-1]), (x[:1].ravel(), aux[:0]),
                 (np.r_[x[0, :8], np.float32(len(gl.materials()))], aux), (np.r_[x[0, :8], np.float32(-1)], aux),
                 (np.r_[x[0, :8], np.float32(0.5)], aux)]
        for xr, a in cases:
            xr = np.ascontiguousarray(xr, np.float32)
            st = g.lib.bre_device_check(g.h, 13, xr.size, xr.ctypes.data, a.size, a.ctypes.data if a.size else None,
                                        y.ctypes.data)
            assert st == 1, (xr, a.size)


# ---------------- 2. photon pass ----------------
@pytest.mark.parametrize("form", [1, 2, 0], ids=["default", "two-slot", "two-trace"])
@pytest.mark.parametrize("iteration", gs.PHOTON_ITERATIONS)
@pytest.mark.parametrize("name", gs.NAMES)
def test_photon_pass_bit_exact(bre, name, iteration, form):
    case = gs.build(name)
    ref, _, _ = gr.photon_ref(name, iteration)
    with bre.BeamGather(0) as g:
        g.set_option(116, form)
        gs.apply(g, case)
        n = g.trace_photons(case.scene, gs.N_PHOTONS, iteration, gs.MAX_DEPTH, gs.RADIUS)
        got = g.get_beams()
        assert n == int(ref["counts"].sum())
        for k in BEAM_KEYS:
            assert np.array_equal(bits(got[k]), bits(ref[k])), k
        if iteration == 0 and form == 1:
            # per-photon counts: at iteration 0 photon i draws from sequence i + 1 whatever the pass's size; the
            # sizes straddle a wave, where the slot copy can go wrong
            cum = np.cumsum(ref["counts"])
            for k in (1, 2, 3, 5, 17, 64, 65, 127, 200, 1999):
                assert g.trace_photons(case.scene, k, 0, gs.MAX_DEPTH, gs.RADIUS) == int(cum[k - 1]), k


@pytest.mark.parametrize("name", ["plastic", "mixed"])
def test_photon_pass_at_the_deepest_maxdepth(bre, scene_mod_gpu, name):
    """maxdepth 16 (BRE_MAX_DEPTH): the glossy kernels keep their suspended frames in the block's LDS, sized by
    maxdepth; this is the largest region, and the longest stack of frames, a launch can ask for."""
    case = gs.build(name)
    depth, n = scene_mod_gpu.MAX_DEPTH, gr.DEEP_PHOTONS
    ref, _ = gr.deep_photon_ref(name, depth)  # (its normal-incidence samples are in the margin check too)
    assert ref["counts"].max() > 8  # paths that go deeper than the other tests' maxdepth 5
    with bre.BeamGather(0) as g:
        gs.apply(g, case)
        assert g.trace_photons(case.scene, n, 0, depth, gs.RADIUS) == int(ref["counts"].sum())
        got = g.get_beams()
    for k in BEAM_KEYS:
        assert np.array_equal(bits(got[k]), bits(ref[k])), k


# ---------------- 3. camera pass ----------------
def _sorted(seg):
    order = np.lexsort((seg["depth"], seg["pixel"]))
    return {k: seg[k][order] for k in ("o", "p", "d", "tmax", "pixel", "depth")}


def _camera(bre, case, iteration):
    import torch

    surf = torch.zeros((gs.CAM_W * gs.CAM_H, 3), dtype=torch.float32, device="cuda")
    with bre.BeamGather(0) as g:
        gs.apply(g, case)
        n = g.camera_pass(case.scene, gs.CAM_W, gs.CAM_H, iteration, gs.CAM_DEPTH, surface=surf)
        seg = g.get_segments()
    torch.cuda.synchronize()
    return n, seg, surf.cpu().numpy()


@pytest.mark.parametrize("iteration", gs.CAMERA_ITERATIONS)
@pytest.mark.parametrize("name", gs.NAMES)
def test_camera_pass_bit_exact(bre, name, iteration):
    """Segments and surface radiance, bit for bit: both EstimateDirect halves through BSDF::f, Pdf and Sample_f."""
    ref, _, _ = gr.camera_ref(name, iteration)
    n, gpu, surf = _camera(bre, gs.build(name), iteration)
    assert n == gpu["o"].shape[0] == ref["o"].shape[0]
    a, r = _sorted(gpu), _sorted(ref)
    assert np.array_equal(a["pixel"], r["pixel"]) and np.array_equal(a["depth"], r["depth"])
    for k in ("o", "p", "d", "tmax"):
        assert np.array_equal(bits(a[k]), bits(r[k])), k
    assert np.array_equal(bits(surf), bits(ref["surface"]))


# ---------------- 4. one lobe is the lobe ----------------
def test_onelobe_equals_matte_context(bre):
    """A plastic with Ks 0 and Kd = k, and a matte entry with sigma 0, give the bits of the triangles' own kd."""
    a, b = gs.build("onelobe"), gs.build("onelobe_plain")
    assert a.tri_mat != b.tri_mat
    beams = []
    for case in (a, b):
        with bre.BeamGather(0) as g:
            gs.apply(g, case)
            g.trace_photons(case.scene, gs.N_PHOTONS, 0, gs.MAX_DEPTH, gs.RADIUS)
            beams.append(g.get_beams())
    assert beams[0]["radius"].shape[0] > gs.N_PHOTONS
    for k in BEAM_KEYS:
        assert np.array_equal(bits(beams[0][k]), bits(beams[1][k])), k
    (na, sa, fa), (nb, sb, fb) = _camera(bre, a, 0), _camera(bre, b, 0)
    assert na == nb > 0 and fa.max() > 0
    for k in ("o", "p", "d", "tmax", "pixel", "depth"):
        assert np.array_equal(sa[k].view(np.uint32), sb[k].view(np.uint32)), k
    assert np.array_equal(bits(fa), bits(fb))


# ---------------- 5. whole iteration ----------------
def _render_iteration(g, scene, params):
    import torch

    ld = torch.zeros((params.width * params.height, 3), dtype=torch.float32, device="cuda")
    g.render_iteration(scene, params, 0, ld)
    torch.cuda.synchronize()
    return ld.cpu().numpy()


@pytest.mark.parametrize("name", ["metal", "mixed"])
def test_render_iteration(bre, oracle, scene_mod_gpu, name):
    case = gs.build(name)
    w = h = 24
    R = 0.05
    p = scene_mod_gpu.render_params(w, h, iterations=1, photons=gs.N_PHOTONS, max_depth=5, radius=R, alpha=0.5)
    sc = gr.scene(name)
    beams = rpb.trace_photons(sc, gs.N_PHOTONS, 0, 5, R)
    cam, _, _ = gr.camera_ref(name, 0)
    bf = oracle.bruteforce(beams, cam, R)
    ref = cam["surface"].astype(np.float64)
    np.add.at(ref, cam["pixel"], bf["seg_rgb_exact"])
    with bre.BeamGather(0) as g:
        gs.apply(g, case)
        got = _render_iteration(g, case.scene, p)
    print(f"{name} 24x24 iteration: rel-L2 {rel_l2(got, ref):.3e}")
    assert ref.max() > 0
    assert_image_bar(got, ref)


# ---------------- 6. context walk ----------------
def test_context_walk_wide_and_narrow_tables(bre, scene_mod_gpu):
    sm = scene_mod_gpu
    case = gs.build("metal")
    narrow = specular_scenes.build("prism")  # the same walls, spot and triangle count, a narrow table
    assert narrow[0].n_triangles == case.scene.n_triangles and not any(isinstance(m, sm.MaterialEx) for m in narrow[2])
    p = sm.render_params(24, 24, iterations=1, photons=gs.N_PHOTONS, max_depth=5, radius=0.05, alpha=0.5)

    def fresh(mats, tri_mat):
        with bre.BeamGather(0) as g:
            g.set_lights(case.lights)
            g.set_materials(mats, tri_mat)
            return _render_iteration(g, case.scene, p)

    matte, shiny, prism = fresh([], []), fresh(case.materials, case.tri_mat), fresh(narrow[2], narrow[3])
    assert matte.max() > 0 and rel_l2(shiny, matte) > 1e-3 and rel_l2(prism, shiny) > 1e-3
    with bre.BeamGather(0) as g:
        g.set_lights(case.lights)
        g.set_materials(case.materials, case.tri_mat)
        assert_image_bar(_render_iteration(g, case.scene, p), shiny, l2=1e-6)
        g.set_materials()  # cleared: the matte kernels again, and the cache key without a table
        assert_image_bar(_render_iteration(g, case.scene, p), matte, l2=1e-6)
        g.set_materials(narrow[2], narrow[3])  # narrow, then wide, then narrow: the last one wins
        assert_image_bar(_render_iteration(g, case.scene, p), prism, l2=1e-6)
        g.set_materials(case.materials, case.tri_mat)
        assert_image_bar(_render_iteration(g, case.scene, p), shiny, l2=1e-6)
        g.set_materials(narrow[2], narrow[3])
        assert_image_bar(_render_iteration(g, case.scene, p), prism, l2=1e-6)
        # a refused table leaves the context as it was
        with pytest.raises(bre.BreError) as e:
            g.set_materials([sm.plastic(0.5, 0.5, 0.0)], [0] * case.scene.n_triangles)
        assert e.value.status == 1 and "material" in str(e.value)
        assert_image_bar(_render_iteration(g, case.scene, p), prism, l2=1e-6)


# ---------------- 7. sharded ----------------
@pytest.mark.parametrize("shards", [1, 2])
def test_render_sharded_with_wide_table(bre, scene_mod_gpu, shards):
    case = gs.build("metal")
    p = scene_mod_gpu.render_params(24, 24, iterations=2, photons=gs.N_PHOTONS, max_depth=5, radius=0.05, alpha=0.5)
    with bre.BeamGather(0) as g:
        gs.apply(g, case)
        whole = g.render(case.scene, p)
    ctxs = [bre.BeamGather(0) for _ in range(shards)]
    try:
        for c in ctxs[:-1]:
            gs.apply(c, case)
        if shards > 1:
            ctxs[-1].set_lights(case.lights)
            with pytest.raises(bre.BreError) as e:  # films of differently shaded scenes would be summed
                bre.render_sharded(ctxs, case.scene, p)
            assert e.value.status == 1 and "materials" in str(e.value)
        gs.apply(ctxs[-1], case)
        img = bre.render_sharded(ctxs, case.scene, p)
    finally:
        for c in ctxs:
            c.close()
    assert whole.max() > 0 and rel_l2(img, whole) <= 1e-6


# ---------------- 8. the wide setter's arguments ----------------
def test_set_materials_ex_refusals(bre, scene_mod_gpu):
    """Each BRE_ERR_INVALID_ARG case of bre_set_materials_ex; the message names the material and the context keeps
    what it holds."""
    import ctypes

    sm = scene_mod_gpu
    case = gs.build("plastic")
    n = case.scene.n_triangles
    nan, inf = float("nan"), float("inf")

    def reserved(k):
        m = sm.plastic()
        m.reserved[k] = 1
        return m

    unknown = sm.plastic()
    unknown.type = 7
    zero_type = sm.plastic()
    zero_type.type = 0
    remap2 = sm.plastic()
    remap2.remap = 2
    bad = [unknown, zero_type, remap2, reserved(0), reserved(2),
           sm.plastic(nan, 0.5), sm.plastic(0.5, inf), sm.plastic(0.5, 0.5, nan), sm.plastic(0.5, 0.5, 0.0),
           sm.plastic(0.5, 0.5, -0.1), sm.matte(nan, 10.0), sm.matte(0.5, inf),
           sm.metal((0.2, 0.0, 1.1), 3.0), sm.metal(nan, 3.0), sm.metal(0.2, inf), sm.metal(0.2, 3.0, 0.0),
           sm.metal(0.2, 3.0, 0.01, -0.1), sm.metal(0.2, 3.0, 0.0, 0.1, 0.0), sm.metal(0.2, 3.0, nan),
           sm.widen(sm.glass(1, 1, 0.0)), sm.widen(sm.interface())]  # (an interface needs bre_set_media first)
    with bre.BeamGather(0) as g:
        gs.apply(g, case)
        before = g.trace_photons(case.scene, 500, 0, 5, 0.05)
        for m in bad:
            with pytest.raises(bre.BreError) as e:
                g.set_materials([m], [0] * n)
            assert e.value.status == 1 and "material 0" in str(e.value), str(e.value)
        for bad_map in ([len(case.materials)] + [-1] * (n - 1), [-2] + [-1] * (n - 1)):
            with pytest.raises(bre.BreError):
                g.set_materials(case.materials, bad_map)
        arr = (sm.MaterialEx * len(case.materials))(*case.materials)
        tm = np.array(case.tri_mat, np.int32)
        assert g.lib.bre_set_materials_ex(g.h, None, len(case.materials), tm.ctypes.data, n) == 1
        assert g.lib.bre_set_materials_ex(g.h, arr, len(case.materials), None, n) == 1
        assert g.lib.bre_set_materials_ex(g.h, arr, -1, tm.ctypes.data, n) == 1
        assert g.lib.bre_set_materials_ex(g.h, arr, sm.MAX_MATERIALS + 1, tm.ctypes.data, n) == 1
        assert g.lib.bre_set_materials_ex(g.h, arr, len(case.materials), tm.ctypes.data, -1) == 1
        # the narrow setter does not know the wide types
        narrow = sm.Material(sm.MATERIAL_PLASTIC, sm.F3(), sm.F3(), 1.5)
        assert g.lib.bre_set_materials(g.h, ctypes.byref(narrow), 1, tm.ctypes.data, n) == 1
        assert g.trace_photons(case.scene, 500, 0, 5, 0.05) == before
        # accepted: colours outside [0, 1] are clamped, a uroughness of 0 falls back, a metal k of 0
        g.set_materials([sm.plastic(1.5, -0.5, 0.2), sm.metal(1.5, 0.0, 0.2, 0.0, 0.3)], [0] + [1] * (n - 1))
        assert g.trace_photons(case.scene, 500, 0, 5, 0.05) > 0
        # the other triangle count is refused at the pass
        other = sm.make_scene(sm.cornell_meshes()[:-2], 0.05, 0.5, 0.0)
        with pytest.raises(bre.BreError) as e:
            g.trace_photons(other, 100, 0, 5, 0.05)
        assert e.value.status == 1 and "material" in str(e.value)


# ---------------- 9. .pbrt ----------------
def test_pbrt_glossy_fog_equals_library_render(bre):
    """bre_pbrt on scenes/glossy_fog.pbrt at 64 x 48, 3 iterations, 20k photons: the library render of the hand-built
    scene (the parse itself is held to it byte for byte in tests/test_glossy_refpy.py)."""
    import importlib
    import os

    pb = importlib.import_module("beam-radiance-estimate-pbrt_amd.pbrt")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "scenes", "glossy_fog.pbrt")).read()
    text = (text.replace("[256]", "[64]", 1).replace("[256]", "[48]", 1).replace("[50000]", "[20000]")
            .replace('"integer iterations" [32]', '"integer iterations" [3]')
            .replace('"float initialbeamradius" [0.01]', '"float initialbeamradius" [0.05]'))
    s = pb.parse_string(text)
    assert s.ok and s.n_errors == 0 and len(s.lights) == 1 and len(s.materials_ex) == 5, s.messages
    assert (s.params.width, s.params.height, s.params.iterations, s.params.photons_per_iteration) == (64, 48, 3, 20000)
    img = s.render(write_files=False)
    case = gs.build("glossy_fog")
    with bre.BeamGather(0) as g:
        gs.apply(g, case)
        L = g.render(case.scene, s.params)
        g.set_materials()
        L_matte = g.render(case.scene, s.params)
    ref = pb.film_finalize(L.reshape(-1, 3), s.film["scale"]).reshape(L.shape)
    assert img.shape == (48, 64, 3) and img.max() > 0
    assert rel_l2(L, L_matte) > 1e-3  # the file's materials reached the render
    assert_image_bar(img, ref)
    # two contexts on one device: the wide table is set on both
    assert rel_l2(s.render(devices=[0, 0], write_files=False), img) <= 1e-6
