"""Point and spot lights on the GPU (bre_set_lights) against the pure-Python float32 restatement
tests/refpy_passes.py (photon pass and camera pass), bit for bit, and the
whole iteration, the context walk, the sharded render and the .pbrt front end to the project's image bar
(relative L2 <= 1e-5, every pixel above 1e-3 of the maximum within 1e-4).

The restatement is the slow side: each reference is computed once per (scene, iteration) and shared
(tests/pass_refs.py).
"""
import functools
import importlib

import numpy as np
import pytest

import lights_scenes as ls
import pass_refs
import refpy_passes as rpass
from lights_scenes import CAM_DEPTH, CAM_H, CAM_W, MAX_DEPTH, N_PHOTONS, RADIUS

pytestmark = pytest.mark.gpu

BEAM_KEYS = ("start", "end", "radius", "power")


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return ls.build(name)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------- 1. photon pass ----------------
@pytest.mark.parametrize("form", [1, 2, 0], ids=["default", "two-slot", "two-trace"])
@pytest.mark.parametrize("iteration", ls.PHOTON_ITERATIONS)
@pytest.mark.parametrize("name", ls.PHOTON_NAMES)
def test_photon_pass_bit_exact(bre, name, iteration, form):
    scene, lights = scene_of(name)
    ref, _ = pass_refs.photon_ref(ls, name, iteration)
    infos = ref["infos"]
    if name == "spot":  # the cone's flat part and its falloff band are both exercised
        fo = [float(i["falloff"]) for i in infos]
        assert any(f == 1.0 for f in fo) and any(0.0 < f < 1.0 for f in fo)
    if name == "floor":
        assert (ref["counts"] == 0).sum() > 10  # photons that escape leave no beam
    if name == "mixed":
        kinds = {i["light"] for i in infos}
        assert 1 not in kinds and {0, 2, 3, 4} <= kinds  # the I = 0 spot is never chosen, all others are
    with bre.BeamGather(0) as g:
        g.set_option(116, form)
        g.set_lights(lights)
        n = g.trace_photons(scene, N_PHOTONS, iteration, MAX_DEPTH, RADIUS)
        got = g.get_beams()
        assert n == int(ref["counts"].sum())
        for k in BEAM_KEYS:
            assert np.array_equal(bits(got[k]), bits(ref[k])), k
        if iteration == 0 and form == 1:
            # per-photon counts: at iteration 0 photon i draws from sequence i + 1 whatever the pass's
            # size, so a pass of the first k photons must hold exactly the first k photons' beams
            cum = np.cumsum(ref["counts"])
            for k in (1, 2, 3, 5, 17, 64, 65, 127, 200):
                assert g.trace_photons(scene, k, 0, MAX_DEPTH, RADIUS) == int(cum[k - 1]), k


# ---------------- 2. camera pass ----------------
def _sorted(seg):
    order = np.lexsort((seg["depth"], seg["pixel"]))
    return {k: seg[k][order] for k in ("o", "p", "d", "tmax", "pixel", "depth")}


def _camera(bre, scene, lights, iteration):
    import torch

    surf = torch.zeros((CAM_W * CAM_H, 3), dtype=torch.float32, device="cuda")
    with bre.BeamGather(0) as g:
        g.set_lights(lights)
        n = g.camera_pass(scene, CAM_W, CAM_H, iteration, CAM_DEPTH, surface=surf)
        seg = g.get_segments()
    torch.cuda.synchronize()
    assert n == seg["o"].shape[0]
    seg["surface"] = surf.cpu().numpy()
    return seg


@pytest.mark.parametrize("iteration", ls.CAMERA_ITERATIONS)
@pytest.mark.parametrize("name", ls.CAMERA_NAMES)
def test_camera_pass_bit_exact(bre, name, iteration):
    """Segments (a missing shadow-ray Tr in the grid medium would shift the sampler's dimensions and so
    the bounce segments) and surface radiance, bit for bit."""
    scene, lights = scene_of(name)
    ref, stats = pass_refs.camera_ref(ls, name, iteration)
    if name == "blocker":  # some shadow rays are blocked, some reach the light
        assert stats["shadow_blocked"] > 0 and stats["shadow_clear"] > 0
    if name == "floor":  # camera rays that miss the quad leave their pixels at 0
        assert 0 < len(set(ref["pixel"].tolist())) < CAM_W * CAM_H
        assert (ref["surface"].max(axis=1) == 0).any() and ref["surface"].max() > 0
    gpu = _camera(bre, scene, lights, iteration)
    assert gpu["o"].shape[0] == ref["o"].shape[0]
    g, r = _sorted(gpu), _sorted(ref)
    assert np.array_equal(g["pixel"], r["pixel"]) and np.array_equal(g["depth"], r["depth"])
    for k in ("o", "p", "d", "tmax"):
        assert np.array_equal(bits(g[k]), bits(r[k])), k
    assert np.array_equal(bits(gpu["surface"]), bits(ref["surface"]))


# ---------------- 3. whole iteration ----------------
def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def assert_image_bar(got, ref, l2=1e-5):
    """relative L2 <= 1e-5, every pixel above 1e-3 of the maximum within 1e-4."""
    got, ref = np.asarray(got, np.float64).reshape(-1, 3), np.asarray(ref, np.float64).reshape(-1, 3)
    assert rel_l2(got, ref) <= l2, rel_l2(got, ref)
    bright = ref.max(axis=1) > 1e-3 * ref.max()
    assert (np.abs(got - ref)[bright] <= 1e-4 * np.abs(ref[bright]).max(axis=1, keepdims=True)).all()


def _render_iteration(bre, g, scene, params):
    import torch

    ld = torch.zeros((params.width * params.height, 3), dtype=torch.float32, device="cuda")
    g.render_iteration(scene, params, 0, ld)
    torch.cuda.synchronize()
    return ld.cpu().numpy()


def test_render_iteration_spot_fog(bre, oracle, scene_mod_gpu):
    scene, lights = scene_of("spot")
    w = h = 32
    R = 0.05
    p = scene_mod_gpu.render_params(w, h, iterations=1, photons=2000, max_depth=5, radius=R, alpha=0.5)
    sc = pass_refs.scene(ls, "spot")
    beams = rpass.trace_photons(sc, 2000, 0, 5, R)
    cam = rpass.camera_pass(sc, w, h, 0, 5)
    bf = oracle.bruteforce(beams, cam, R)
    ref = cam["surface"].astype(np.float64)
    np.add.at(ref, cam["pixel"], bf["seg_rgb_exact"])
    with bre.BeamGather(0) as g:
        g.set_lights(lights)
        got = _render_iteration(bre, g, scene, p)
    print(f"spot_fog 32x32 iteration: rel-L2 {rel_l2(got, ref):.3e}")
    assert_image_bar(got, ref)
    lit = cam["surface"].max(axis=1) > 0  # the cone's footprint on the walls, as the camera sees it
    assert lit.sum() > 10 and (got[lit].max(axis=1) > 0).all()


# ---------------- 4. context walk ----------------
def test_context_walk_set_and_clear_lights(bre, scene_mod_gpu):
    spot_scene, lights = scene_of("spot")
    cornell = scene_mod_gpu.cornell_scene()
    p = scene_mod_gpu.render_params(32, 32, iterations=1, photons=3000, max_depth=5, radius=0.05, alpha=0.5)
    with bre.BeamGather(0) as fresh:
        want_cornell = _render_iteration(bre, fresh, cornell, p)
    with bre.BeamGather(0) as g:
        g.set_lights(lights)
        first = _render_iteration(bre, g, spot_scene, p)
        assert first.max() > 0
        g.set_lights([])
        assert_image_bar(_render_iteration(bre, g, cornell, p), want_cornell, l2=1e-6)
        # neither lights nor an emitter: refused, and the context stays usable
        with pytest.raises(bre.BreError) as e:
            g.trace_photons(spot_scene, 100, 0, 5, 0.05)
        assert e.value.status == 1 and "no area light" in str(e.value)
        g.set_lights(lights)
        assert_image_bar(_render_iteration(bre, g, spot_scene, p), first, l2=1e-6)
        # an order beyond the scene's triangles is refused by the pass
        late = scene_mod_gpu.spot_light(ls.SPOT_FROM, ls.SPOT_TO, ls.SPOT_I, order=spot_scene.n_triangles + 1)
        g.set_lights([late])
        for call in (lambda: g.trace_photons(spot_scene, 100, 0, 5, 0.05), lambda: g.camera_pass(spot_scene, 16, 16)):
            with pytest.raises(bre.BreError) as e:
                call()
            assert e.value.status == 1 and "order" in str(e.value)
        g.set_lights(lights)
        assert_image_bar(_render_iteration(bre, g, spot_scene, p), first, l2=1e-6)


# ---------------- 5. sharded ----------------
def test_render_sharded_with_lights(bre, scene_mod_gpu):
    scene, lights = scene_of("spot")
    p = scene_mod_gpu.render_params(32, 32, iterations=2, photons=3000, max_depth=5, radius=0.05, alpha=0.5)
    with bre.BeamGather(0) as g:
        g.set_lights(lights)
        whole = g.render(scene, p)
    with bre.BeamGather(0) as a, bre.BeamGather(0) as b:
        a.set_lights(lights)
        with pytest.raises(bre.BreError) as e:  # films of different scenes would be summed
            bre.render_sharded([a, b], scene, p)
        assert e.value.status == 1 and "lights" in str(e.value)
        b.set_lights(lights)
        img = bre.render_sharded([a, b], scene, p)
    assert whole.max() > 0 and rel_l2(img, whole) <= 1e-6


# ---------------- 6. .pbrt ----------------
def test_pbrt_spot_fog_equals_library_render(bre):
    import os

    pb = importlib.import_module("beam-radiance-estimate-pbrt_amd.pbrt")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "scenes", "spot_fog.pbrt")).read()
    text = (text.replace("[256]", "[40]", 1).replace("[256]", "[32]", 1).replace("[50000]", "[20000]")
            .replace('"float initialbeamradius" [0.01]', '"float initialbeamradius" [0.05]'))
    s = pb.parse_string(text, quick=True)
    assert s.ok and s.n_errors == 0 and len(s.lights) == 1, s.messages
    img = s.render(write_files=False)
    with bre.BeamGather(0) as g:
        g.set_lights(s.lights)
        L = g.render(s.scene, s.params)
    ref = pb.film_finalize(L.reshape(-1, 3), s.film["scale"]).reshape(L.shape)
    assert img.shape == (32, 40, 3) and img.max() > 0
    assert_image_bar(img, ref)
    # two contexts on one device (bre_pbrt_render_devices): the lights are set on both
    assert rel_l2(s.render(devices=[0, 0], write_files=False), img) <= 1e-6


# ---------------- bre_set_lights refusals on a live context ----------------
def test_set_lights_refusals_leave_the_lights_unchanged(bre, scene_mod_gpu):
    sm = scene_mod_gpu
    scene, lights = scene_of("spot")
    good = lights[0]

    def variant(**kw):
        L = sm.Light.from_buffer_copy(good.to_bytes())
        for k, v in kw.items():
            if isinstance(v, tuple):
                arr = getattr(L, k)
                arr[v[0]] = v[1]
            else:
                setattr(L, k, v)
        return L

    with bre.BeamGather(0) as g:
        g.set_lights(lights)
        want = g.trace_photons(scene, 500, 0, 5, 0.01)
        assert want > 0
        bad = [variant(type=0), variant(type=3), variant(order=-1), variant(I=(1, float("nan"))),
               variant(light_to_world=(5, float("inf"))), variant(world_to_light=(0, float("nan"))),
               variant(cone_total_deg=float("inf")), variant(cone_falloff_start_deg=float("nan"))]
        for L in bad:
            with pytest.raises(bre.BreError) as e:
                g.set_lights([good, L])
            assert e.value.status == 1 and "light 1" in str(e.value)
        with pytest.raises(bre.BreError) as e:
            g.set_lights([good] * (sm.MAX_LIGHTS + 1))
        assert e.value.status == 1
        assert g.lib.bre_set_lights(g.h, None, 1) == 1 and g.lib.bre_set_lights(g.h, None, -1) == 1
        # every refusal left the context's lights as they were
        assert g.trace_photons(scene, 500, 0, 5, 0.01) == want
        g.set_lights([good] * sm.MAX_LIGHTS)  # the cap itself is accepted
        assert g.trace_photons(scene, 500, 0, 5, 0.01) > 0
