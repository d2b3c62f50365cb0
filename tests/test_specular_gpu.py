"""Mirror and glass on the GPU (bre_set_materials, bre_device_check kind 12) against the pure-Python float32
restatement (tests/refpy_specular.py, tests/refpy_passes.py), bit for bit: the lobe on its own, the two passes
on the scenes of tests/specular_scenes.py.  The whole iteration, the context walk, the sharded render and
the .pbrt front end are held to the project's image bar (relative L2 <= 1e-5, every pixel
above 1e-3 of the maximum within 1e-4).

The restatement is the slow side: tests/pass_refs.py computes each reference once per (scene, iteration).
"""
import importlib
import os

import numpy as np
import pytest

import pass_refs
import refpy_passes as rpass
import refpy_specular as rs
import specular_scenes as ss
from refpy_photon import ONE_MINUS_EPS

pytestmark = pytest.mark.gpu

BEAM_KEYS = ("start", "end", "radius", "power")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


# ---------------- 1. the lobe on its own (kind 12) ----------------
ETAS = (0.0, 1.0, 1.33, 1.5, 2.4)  # 0: the mirror


def lobe_records():
    """~50k records: wo on a grid of the sphere (wo.z = 0, +-1 and grazing included), u0 at 0, just below F, at F,
    just above F, 0.5 and OneMinusEpsilon, every eta and the mirror, both modes."""
    f32 = np.float32
    zs = np.concatenate([[-1.0, 1.0, 0.0, -0.0, 1e-3, -1e-3, 1e-6, -1e-6, 0.999, -0.999],
                         np.linspace(-0.98, 0.98, 43)]).astype(np.float32)
    phis = (np.arange(16, dtype=np.float32) + f32(0.25)) * f32(2 * np.pi / 16)
    rec = []
    for z in zs:
        s = f32(np.sqrt(max(f32(0), f32(1) - z * z)))
        for phi in phis:
            wo = (f32(s * np.cos(phi)), f32(s * np.sin(phi)), f32(z))
            for eta in ETAS:
                F = f32(0.5) if eta == 0 else rs.fr_dielectric(wo[2], f32(1), f32(eta))[0]
                us = (f32(0), np.nextafter(F, f32(-1)), F, np.nextafter(F, f32(2)), f32(0.5), ONE_MINUS_EPS)
                for u0 in us:
                    u0 = min(max(f32(u0), f32(0)), ONE_MINUS_EPS)  # a sampler's range
                    for mode in (0.0, 1.0):
                        rec.append((wo[0], wo[1], wo[2], u0, eta, mode))
    return np.array(rec, np.float32)


def test_specular_lobe_bit_exact(bre):
    x = lobe_records()
    assert 45000 <= x.shape[0] <= 60000
    ref = np.zeros((x.shape[0], 6), np.float32)
    typ = np.zeros(x.shape[0], np.int32)
    branches = {}
    for i, r in enumerate(x):
        m = rs.Mat(rs.MIRROR if r[4] == 0 else rs.GLASS, (1, 1, 1), (1, 1, 1), r[4])
        wi, pdf, f, t, branch = rs.specular_sample(m, r[:3], r[3], rs.RADIANCE if r[5] else rs.IMPORTANCE)
        ref[i, :3], ref[i, 3], ref[i, 4], typ[i] = wi, pdf, f[0], t
        branches[branch] = branches.get(branch, 0) + 1
    for b in ("wo_z0", "mirror_reflect", "glass_reflect", "tir", "transmit_enter", "transmit_leave"):
        assert branches.get(b, 0) > 50, (b, branches)
    with bre.BeamGather(0) as g:
        wi, pdf, f, t = g.specular_check(x)
    assert np.array_equal(t, typ)
    assert np.array_equal(bits(wi), bits(ref[:, :3]))
    assert np.array_equal(bits(pdf), bits(ref[:, 3]))
    assert np.array_equal(bits(f), bits(ref[:, 4]))
    with bre.BeamGather(0) as g:  # whole records only
        with pytest.raises(bre.BreError) as e:
            g.device_check(12, np.zeros(7, np.float32))
        assert e.value.status == 1


# ---------------- 2. photon pass ----------------
@pytest.mark.parametrize("form", [1, 2, 0], ids=["default", "two-slot", "two-trace"])
@pytest.mark.parametrize("iteration", ss.PHOTON_ITERATIONS)
@pytest.mark.parametrize("name", ss.NAMES)
def test_photon_pass_bit_exact(bre, name, iteration, form):
    scene, lights, mats, tri_mat = ss.build(name)
    ref, _ = pass_refs.photon_ref(ss, name, iteration)
    with bre.BeamGather(0) as g:
        g.set_option(116, form)
        g.set_lights(lights)
        g.set_materials(mats, tri_mat)
        n = g.trace_photons(scene, ss.N_PHOTONS, iteration, ss.MAX_DEPTH, ss.RADIUS)
        got = g.get_beams()
        assert n == int(ref["counts"].sum())
        for k in BEAM_KEYS:
            assert np.array_equal(bits(got[k]), bits(ref[k])), k
        if iteration == 0 and form == 1:
            # per-photon counts: at iteration 0 photon i draws from sequence i + 1 whatever the pass's size
            cum = np.cumsum(ref["counts"])
            for k in (1, 2, 3, 5, 17, 64, 65, 127, 200, 1999):
                assert g.trace_photons(scene, k, 0, ss.MAX_DEPTH, ss.RADIUS) == int(cum[k - 1]), k


# ---------------- 3. camera pass ----------------
def _sorted(seg):
    order = np.lexsort((seg["depth"], seg["pixel"]))
    return {k: seg[k][order] for k in ("o", "p", "d", "tmax", "pixel", "depth")}


@pytest.mark.parametrize("iteration", ss.CAMERA_ITERATIONS)
@pytest.mark.parametrize("name", ss.CAMERA_NAMES)
def test_camera_pass_bit_exact(bre, name, iteration):
    """Segments (a Tr draw on a specular vertex in the grid medium would shift the sampler's dimensions and so
    the later segments) and surface radiance, bit for bit."""
    import torch

    scene, lights, mats, tri_mat = ss.build(name)
    ref, _ = pass_refs.camera_ref(ss, name, iteration)
    surf = torch.zeros((ss.CAM_W * ss.CAM_H, 3), dtype=torch.float32, device="cuda")
    with bre.BeamGather(0) as g:
        g.set_lights(lights)
        g.set_materials(mats, tri_mat)
        n = g.camera_pass(scene, ss.CAM_W, ss.CAM_H, iteration, ss.CAM_DEPTH, surface=surf)
        gpu = g.get_segments()
    torch.cuda.synchronize()
    assert n == gpu["o"].shape[0] == ref["o"].shape[0]
    a, r = _sorted(gpu), _sorted(ref)
    assert np.array_equal(a["pixel"], r["pixel"]) and np.array_equal(a["depth"], r["depth"])
    for k in ("o", "p", "d", "tmax"):
        assert np.array_equal(bits(a[k]), bits(r[k])), k
    assert np.array_equal(bits(surf.cpu().numpy()), bits(ref["surface"]))


# ---------------- 4. whole iteration ----------------
def _render_iteration(g, scene, params):
    import torch

    ld = torch.zeros((params.width * params.height, 3), dtype=torch.float32, device="cuda")
    g.render_iteration(scene, params, 0, ld)
    torch.cuda.synchronize()
    return ld.cpu().numpy()


def test_render_iteration_prism(bre, oracle, scene_mod_gpu):
    scene, lights, mats, tri_mat = ss.build("prism")
    w = h = 32
    R = 0.05
    p = scene_mod_gpu.render_params(w, h, iterations=1, photons=3000, max_depth=5, radius=R, alpha=0.5)
    sc = pass_refs.scene(ss, "prism")
    beams = rpass.trace_photons(sc, 3000, 0, 5, R)
    cam = rpass.camera_pass(sc, w, h, 0, 5)
    bf = oracle.bruteforce(beams, cam, R)
    ref = cam["surface"].astype(np.float64)
    np.add.at(ref, cam["pixel"], bf["seg_rgb_exact"])
    with bre.BeamGather(0) as g:
        g.set_lights(lights)
        g.set_materials(mats, tri_mat)
        got = _render_iteration(g, scene, p)
    print(f"prism 32x32 iteration: rel-L2 {rel_l2(got, ref):.3e}")
    assert ref.max() > 0
    assert_image_bar(got, ref)


# ---------------- 5. context walk ----------------
def test_context_walk_set_and_clear_materials(bre, scene_mod_gpu):
    sm = scene_mod_gpu
    scene, lights, mats, tri_mat = ss.build("prism")
    p = sm.render_params(32, 32, iterations=1, photons=3000, max_depth=5, radius=0.05, alpha=0.5)
    with bre.BeamGather(0) as g:
        g.set_lights(lights)
        matte = _render_iteration(g, scene, p)
        g.set_materials(mats, tri_mat)
        shiny = _render_iteration(g, scene, p)
        assert matte.max() > 0 and rel_l2(shiny, matte) > 1e-3  # the materials change the film
        g.set_materials()
        assert_image_bar(_render_iteration(g, scene, p), matte, l2=1e-6)
        g.set_materials(mats, tri_mat)
        # refusals: the message names the material, and the context keeps what it holds
        M = sm.Material
        n = len(tri_mat)
        bad_tables = [[M(0, sm.F3(), sm.F3(), 1.5)], [M(3, sm.F3(), sm.F3(), 1.5)], [sm.glass(1, 1, 0.0)],
                      [sm.glass(1, 1, -1.5)], [sm.glass(1, 1, float("nan"))], [sm.glass(1, 1, float("inf"))],
                      [sm.mirror(0.9)] * (sm.MAX_MATERIALS + 1)]
        for table in bad_tables:
            with pytest.raises(bre.BreError) as e:
                g.set_materials(table, [0] * n)
            assert e.value.status == 1 and "material" in str(e.value)
        for bad_map in ([len(mats)] + [-1] * (n - 1), [-2] + [-1] * (n - 1)):
            with pytest.raises(bre.BreError) as e:
                g.set_materials(mats, bad_map)
            assert e.value.status == 1 and "material" in str(e.value)
        arr = (M * len(mats))(*mats)
        tm = np.array(tri_mat, np.int32)
        assert g.lib.bre_set_materials(g.h, None, len(mats), tm.ctypes.data, n) == 1
        assert "material" in g.lib.bre_last_error(g.h).decode()
        assert g.lib.bre_set_materials(g.h, arr, len(mats), None, n) == 1
        assert g.lib.bre_set_materials(g.h, arr, -1, tm.ctypes.data, n) == 1
        assert g.lib.bre_set_materials(g.h, arr, len(mats), tm.ctypes.data, -1) == 1
        assert g.lib.bre_set_materials(g.h, arr, len(mats), tm.ctypes.data, sm.MAX_SCENE_TRIANGLES + 1) == 1
        assert_image_bar(_render_iteration(g, scene, p), shiny, l2=1e-6)
        # a scene with another triangle count is refused at the pass; the next good render matches
        other = sm.make_scene(sm.cornell_meshes()[:-1], 0.05, 0.5, 0.0)
        assert other.n_triangles != scene.n_triangles
        for call in (lambda: g.trace_photons(other, 100, 0, 5, 0.05), lambda: g.camera_pass(other, 16, 16)):
            with pytest.raises(bre.BreError) as e:
                call()
            assert e.value.status == 1 and "material" in str(e.value)
        assert_image_bar(_render_iteration(g, scene, p), shiny, l2=1e-6)


# ---------------- 6. sharded ----------------
def test_render_sharded_with_materials(bre, scene_mod_gpu):
    scene, lights, mats, tri_mat = ss.build("prism")
    p = scene_mod_gpu.render_params(32, 32, iterations=2, photons=3000, max_depth=5, radius=0.05, alpha=0.5)
    with bre.BeamGather(0) as g:
        g.set_lights(lights)
        g.set_materials(mats, tri_mat)
        whole = g.render(scene, p)
    with bre.BeamGather(0) as a, bre.BeamGather(0) as b:
        a.set_lights(lights)
        b.set_lights(lights)
        a.set_materials(mats, tri_mat)
        with pytest.raises(bre.BreError) as e:  # films of differently shaded scenes would be summed
            bre.render_sharded([a, b], scene, p)
        assert e.value.status == 1 and "materials" in str(e.value)
        b.set_materials(mats, tri_mat)
        img = bre.render_sharded([a, b], scene, p)
    assert whole.max() > 0 and rel_l2(img, whole) <= 1e-6


# ---------------- 7. .pbrt ----------------
def test_pbrt_prism_fog_equals_library_render(bre):
    pb = importlib.import_module("beam-radiance-estimate-pbrt_amd.pbrt")
    text = open(os.path.join(ROOT, "scenes", "prism_fog.pbrt")).read()
    text = (text.replace("[256]", "[40]", 1).replace("[256]", "[32]", 1).replace("[50000]", "[20000]")
            .replace('"float initialbeamradius" [0.01]', '"float initialbeamradius" [0.05]'))
    s = pb.parse_string(text, quick=True)
    assert s.ok and s.n_errors == 0 and len(s.lights) == 1 and len(s.materials) == 2, s.messages
    img = s.render(write_files=False)
    with bre.BeamGather(0) as g:
        g.set_lights(s.lights)
        g.set_materials(s.materials, s.triangle_material)
        L = g.render(s.scene, s.params)
        g.set_materials()
        L_matte = g.render(s.scene, s.params)
    ref = pb.film_finalize(L.reshape(-1, 3), s.film["scale"]).reshape(L.shape)
    assert img.shape == (32, 40, 3) and img.max() > 0
    assert rel_l2(L, L_matte) > 1e-3  # the file's materials reached the render
    assert_image_bar(img, ref)
    # two contexts on one device (bre_pbrt_render_devices): the materials are set on both
    assert rel_l2(s.render(devices=[0, 0], write_files=False), img) <= 1e-6
