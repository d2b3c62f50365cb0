"""Media bounded by surfaces on the GPU (bre_set_media, BRE_MATERIAL_INTERFACE) against the pure-Python float32
restatement tests/refpy_passes.py, bit for bit: the photon pass in its three forms and the camera pass on the
scenes of tests/media_scenes.py.  The whole iteration, the context walk and the sharded render are held to the
project's image bar (relative L2 <= 1e-5, every pixel above 1e-3 of the maximum within 1e-4).

The restatement is the slow side: tests/pass_refs.py computes each reference once per (scene, iteration).
"""
import numpy as np
import pytest

import media_scenes as ms
import pass_refs
import refpy_passes as rpass

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


# ---------------- 1. photon pass ----------------
@pytest.mark.parametrize("form", [1, 2, 0], ids=["default", "two-slot", "two-trace"])
@pytest.mark.parametrize("iteration", ms.PHOTON_ITERATIONS)
@pytest.mark.parametrize("name", ms.NAMES)
def test_photon_pass_bit_exact(bre, name, iteration, form):
    case = ms.build(name)
    ref, _ = pass_refs.photon_ref(ms, name, iteration)
    with bre.BeamGather(0) as g:
        g.set_option(116, form)
        ms.apply(g, case)
        n = g.trace_photons(case.scene, ms.N_PHOTONS, iteration, ms.MAX_DEPTH, ms.RADIUS)
        got = g.get_beams()
        assert n == int(ref["counts"].sum())
        for k in BEAM_KEYS:
            assert np.array_equal(bits(got[k]), bits(ref[k])), k
        if iteration == 0 and form == 1:
            # per-photon counts: at iteration 0 photon i draws from sequence i + 1 whatever the pass's size
            cum = np.cumsum(ref["counts"])
            for k in (1, 2, 65, 200, 1999):
                assert g.trace_photons(case.scene, k, 0, ms.MAX_DEPTH, ms.RADIUS) == int(cum[k - 1]), k


# ---------------- 2. camera pass ----------------
def _sorted(seg):
    order = np.lexsort((seg["depth"], seg["pixel"]))
    return {k: seg[k][order] for k in ("o", "p", "d", "tmax", "pixel", "depth")}


def _camera(g, case, iteration):
    import torch

    surf = torch.zeros((ms.CAM_W * ms.CAM_H, 3), dtype=torch.float32, device="cuda")
    n = g.camera_pass(case.scene, ms.CAM_W, ms.CAM_H, iteration, ms.CAM_DEPTH, surface=surf)
    gpu = g.get_segments()
    torch.cuda.synchronize()
    assert n == gpu["o"].shape[0]
    return gpu, surf.cpu().numpy()


def assert_camera_equal(gpu, surf, ref):
    assert gpu["o"].shape[0] == ref["o"].shape[0]
    a, r = _sorted(gpu), _sorted(ref)
    assert np.array_equal(a["pixel"], r["pixel"]) and np.array_equal(a["depth"], r["depth"])
    for k in ("o", "p", "d", "tmax"):
        assert np.array_equal(bits(a[k]), bits(r[k])), k
    assert np.array_equal(bits(surf), bits(ref["surface"]))


@pytest.mark.parametrize("iteration", ms.CAMERA_ITERATIONS)
@pytest.mark.parametrize("name", ms.NAMES)
def test_camera_pass_bit_exact(bre, name, iteration):
    """The set of segments, each with its ordinal along the pixel's path, and the surface radiance, bit for bit:
    pixels with more segments than maxdepth included (the default budget holds `slab`'s three crossings)."""
    case = ms.build(name)
    ref, _ = pass_refs.camera_ref(ms, name, iteration)
    with bre.BeamGather(0) as g:
        ms.apply(g, case)
        gpu, surf = _camera(g, case, iteration)
        # the segments leave in (ordinal plane, pixel tile) order
        assert (np.diff(gpu["depth"]) >= 0).all()
    assert_camera_equal(gpu, surf, ref)
    per_pixel = np.bincount(gpu["pixel"], minlength=ms.CAM_W * ms.CAM_H)
    if name in ("box", "camera_in"):
        assert (per_pixel > ms.CAM_DEPTH).any() and gpu["depth"].max() >= ms.CAM_DEPTH


# ---------------- 3. whole iteration ----------------
def _render_iteration(g, scene, params):
    import torch

    ld = torch.zeros((params.width * params.height, 3), dtype=torch.float32, device="cuda")
    g.render_iteration(scene, params, 0, ld)
    torch.cuda.synchronize()
    return ld.cpu().numpy()


def test_render_iteration_nested(bre, oracle, scene_mod_gpu):
    case = ms.build("nested")
    w = h = 32
    R = 0.05
    p = scene_mod_gpu.render_params(w, h, iterations=1, photons=3000, max_depth=5, radius=R, alpha=0.5)
    sc = pass_refs.scene(ms, "nested")
    beams = rpass.trace_photons(sc, 3000, 0, 5, R)
    cam = rpass.camera_pass(sc, w, h, 0, 5)
    bf = oracle.bruteforce(beams, cam, R)
    ref = cam["surface"].astype(np.float64)
    np.add.at(ref, cam["pixel"], bf["seg_rgb_exact"])
    with bre.BeamGather(0) as g:
        ms.apply(g, case)
        got = _render_iteration(g, case.scene, p)
    print(f"nested 32x32 iteration: rel-L2 {rel_l2(got, ref):.3e}")
    assert ref.max() > 0
    assert_image_bar(got, ref)


# ---------------- 4. the segment budget ----------------
def test_segment_budget_overrun_is_reported(bre):
    """`slab`'s paths cross three interfaces: with 2 planes beyond maxdepth the camera pass reports it (a status
    flag, like the traversal stack's), and the context then renders `box` as a fresh one does."""
    slab, box = ms.build("slab"), ms.build("box")
    with bre.BeamGather(0) as g:
        ms.apply(g, slab)
        g.set_option(bre.OPT_SEGMENT_BUDGET, 2)
        with pytest.raises(bre.BreError) as e:
            g.camera_pass(slab.scene, ms.CAM_W, ms.CAM_H, 0, ms.CAM_DEPTH)
        assert e.value.status == 4 and "BRE_OPT_SEGMENT_BUDGET" in str(e.value)  # BRE_ERR_STATE
        g.synchronize()
        ms.apply(g, box)
        g.set_option(bre.OPT_SEGMENT_BUDGET, 16)
        gpu, surf = _camera(g, box, 0)
        assert_camera_equal(gpu, surf, pass_refs.camera_ref(ms, "box", 0)[0])
        for bad in (-1, 241):
            with pytest.raises(bre.BreError):
                g.set_option(bre.OPT_SEGMENT_BUDGET, bad)


# ---------------- 5. context walk ----------------
def test_context_walk_set_and_clear_media(bre, scene_mod_gpu):
    sm = scene_mod_gpu
    case = ms.build("nested")
    fogged = sm.make_scene(ms.meshes_of("nested")[0], 0.05, 0.5, 0.0)  # the same triangles in one medium
    p = sm.render_params(32, 32, iterations=1, photons=3000, max_depth=5, radius=0.05, alpha=0.5)
    n, nl = case.scene.n_triangles, len(case.lights)
    with bre.BeamGather(0) as fresh:
        fresh.set_lights(case.lights)
        one_medium = _render_iteration(fresh, fogged, p)
    with bre.BeamGather(0) as g:
        # an interface material needs the media first
        g.set_lights(case.lights)
        with pytest.raises(bre.BreError) as e:
            g.set_materials(case.materials, case.tri_mat)
        assert e.value.status == 1 and "bre_set_media" in str(e.value)
        ms.apply(g, case)
        with_media = _render_iteration(g, case.scene, p)
        assert with_media.max() > 0
        # clear: the one-medium scene renders a fresh context's bits
        g.set_materials()
        g.set_media()
        assert np.array_equal(bits(_render_iteration(g, fogged, p)), bits(one_medium))
        assert rel_l2(with_media, one_medium) > 1e-3  # the media change the film
        ms.apply(g, case)
        assert np.array_equal(bits(_render_iteration(g, case.scene, p)), bits(with_media))

        # refused at the pass, the context unharmed: a scene with a medium of its own, other counts
        def refused(call, word):
            with pytest.raises(bre.BreError) as e:
                call()
            assert e.value.status == 1 and word in str(e.value), str(e.value)

        for call in (lambda: g.trace_photons(fogged, 100, 0, 5, 0.05), lambda: g.camera_pass(fogged, 16, 16)):
            refused(call, "has_medium")
        other = sm.make_scene(sm.cornell_meshes()[:-1])
        g.set_materials()
        for call in (lambda: g.trace_photons(other, 100, 0, 5, 0.05), lambda: g.camera_pass(other, 16, 16)):
            refused(call, "triangles")
        g.set_lights(list(case.lights) * 2)
        refused(lambda: g.trace_photons(case.scene, 100, 0, 5, 0.05), "delta lights")
        ms.apply(g, case)
        g.set_media()  # the interface triangles are left without media
        refused(lambda: g.camera_pass(case.scene, 16, 16), "bre_set_media")
        ms.apply(g, case)

        # refused at the call, the state left as it was
        M = sm.Medium
        ti, to = list(case.tri_inside), list(case.tri_outside)
        hom, nm = sm.medium_homogeneous, len(case.media)

        def grid(sa=1.0, ss=9.0, g_=0.0, dens=np.ones(8), dims=(2, 2, 2)):
            return sm.medium_grid(sa, ss, g_, dens, dims)

        null_grid = grid()
        null_grid.grid_density = None
        bad_tables = [[M()], [hom(float("nan"), 1.0)], [hom(1.0, float("inf"))], [hom(-0.1, 1.0)], [hom(1.0, (1, -1, 1))],
                      [hom(1.0, 1.0, 1.5)], [hom(1.0, 1.0, float("nan"))], [grid(ss=(9.0, 8.0, 9.0))],
                      [grid(dens=np.zeros(8))], [grid(dens=np.ones(0), dims=(0, 2, 2))], [null_grid],
                      [hom(1.0, 1.0)] * (sm.MAX_MEDIA + 1)]
        for table in bad_tables:
            refused(lambda: g.set_media(table, [0] * n, [0] * n, 0, [0] * nl), "medi")
        refused(lambda: g.set_media(case.media, [nm] + ti[1:], to, -1, [-1] * nl), "index")
        refused(lambda: g.set_media(case.media, ti, [-2] + to[1:], -1, [-1] * nl), "index")
        refused(lambda: g.set_media(case.media, ti, to, nm, [-1] * nl), "camera")
        refused(lambda: g.set_media(case.media, ti, to, -1, [nm] * nl), "light")
        arr = (M * nm)(*case.media)
        a, b = np.array(ti, np.int32), np.array(to, np.int32)
        lm = np.array(case.light_medium, np.int32)
        raw = g.lib.bre_set_media
        assert raw(g.h, None, nm, a.ctypes.data, b.ctypes.data, n, -1, lm.ctypes.data, nl) == 1
        assert raw(g.h, arr, nm, None, b.ctypes.data, n, -1, lm.ctypes.data, nl) == 1
        assert raw(g.h, arr, nm, a.ctypes.data, None, n, -1, lm.ctypes.data, nl) == 1
        assert raw(g.h, arr, nm, a.ctypes.data, b.ctypes.data, n, -1, None, nl) == 1
        assert raw(g.h, arr, -1, a.ctypes.data, b.ctypes.data, n, -1, lm.ctypes.data, nl) == 1
        assert raw(g.h, arr, nm, a.ctypes.data, b.ctypes.data, -1, -1, lm.ctypes.data, nl) == 1
        assert raw(g.h, arr, nm, a.ctypes.data, b.ctypes.data, sm.MAX_SCENE_TRIANGLES + 1, -1, lm.ctypes.data, nl) == 1
        assert raw(g.h, arr, nm, a.ctypes.data, b.ctypes.data, n, -1, lm.ctypes.data, sm.MAX_LIGHTS + 1) == 1
        assert "bre_set_media" in g.lib.bre_last_error(g.h).decode()
        assert np.array_equal(bits(_render_iteration(g, case.scene, p)), bits(with_media))


# ---------------- 6. sharded ----------------
def test_render_sharded_with_media(bre, scene_mod_gpu):
    case = ms.build("nested")
    p = scene_mod_gpu.render_params(32, 32, iterations=2, photons=3000, max_depth=5, radius=0.05, alpha=0.5)
    with bre.BeamGather(0) as g:
        ms.apply(g, case)
        whole = g.render(case.scene, p)
    with bre.BeamGather(0) as a, bre.BeamGather(0) as b:
        ms.apply(a, case)
        ms.apply(b, case)
        # another camera medium: films of differently filled rooms would be summed
        b.set_media(case.media, case.tri_inside, case.tri_outside, -1, case.light_medium)
        with pytest.raises(bre.BreError) as e:
            bre.render_sharded([a, b], case.scene, p)
        assert e.value.status == 1 and "media" in str(e.value)
        ms.apply(b, case)
        img = bre.render_sharded([a, b], case.scene, p)
    assert whole.max() > 0 and rel_l2(img, whole) <= 1e-6


# ---------------- 7. .pbrt ----------------
def test_pbrt_smoke_box_equals_library_render(bre, scene_mod_gpu):
    import ctypes
    import importlib
    import os

    import lights_scenes as ls
    from specular_scenes import box_mesh

    sm = scene_mod_gpu
    pb = importlib.import_module("beam-radiance-estimate-pbrt_amd.pbrt")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "scenes", "smoke_box.pbrt")).read()
    text = (text.replace("[256]", "[40]", 1).replace("[256]", "[32]", 1).replace("[50000]", "[20000]")
            .replace('"integer iterations" [32]', '"integer iterations" [4]')
            .replace('"float initialbeamradius" [0.01]', '"float initialbeamradius" [0.05]'))
    s = pb.parse_string(text, media=True)
    assert s.ok and s.n_errors == 0 and len(s.media) == 2 and s.params.iterations == 4, s.messages
    img = s.render(write_files=False)
    # the same scene built by hand
    smoke, dense = sm.medium_homogeneous(1.0, 8.0, 0.0), sm.medium_homogeneous((4, 2, 1), (12, 18, 24), 0.3)
    meshes = ([m + (None, None) for m in sm.cornell_meshes()[:-1]] +
              [ms.boundary(box_mesh((0.3, 0.25, 0.45), (0.5, 0.5, 0.65), sm.interface()), smoke, None),
               ms.boundary(box_mesh((0.56, 0.25, 0.55), (0.72, 0.45, 0.71), sm.glass(1.0, 1.0, 1.5)), dense, None)])
    hand = sm.make_scene(meshes)
    lights = [sm.spot_light(ls.SPOT_FROM, ls.SPOT_TO, (12.0, 12.0, 12.0), 30.0, 5.0, 0)]
    case = ms.Case(hand, lights, *sm.scene_materials(meshes), *sm.scene_media(meshes, None, [None]))
    used = sm.Scene.triangles.offset + 36 * ctypes.sizeof(sm.Triangle)  # the counts, no medium, the camera, the triangles
    assert hand.to_bytes()[:used] == s.scene.to_bytes()[:used]
    assert [m.to_bytes()[:112] for m in case.media] == [m.to_bytes()[:112] for m in s.media]
    assert list(s.tri_inside) == case.tri_inside and list(s.tri_outside) == case.tri_outside
    with bre.BeamGather(0) as g:
        ms.apply(g, case)
        L = g.render(hand, s.params)
        g.set_materials()
        g.set_media()
        L_bare = g.render(hand, s.params)
    ref = pb.film_finalize(L.reshape(-1, 3), s.film["scale"]).reshape(L.shape)
    assert img.shape == (32, 40, 3) and img.max() > 0
    assert rel_l2(L, L_bare) > 1e-3  # the file's media reached the render
    assert_image_bar(img, ref)
    # two contexts on one device (bre_pbrt_render_devices): the media are set on both
    assert rel_l2(s.render(devices=[0, 0], write_files=False), img) <= 1e-6
