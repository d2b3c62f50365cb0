"""One context walked through every kind of sticky scene state (bre_set_lights, bre_set_media,
bre_set_materials): set, replaced and cleared in turn.  At every stop the photon pass's beams and the camera
pass's segments and surface radiance equal, bit for bit, the pure-Python restatement of that state
(tests/refpy_passes.py); no image is rendered and no run of the library is compared with another.  Then
bre_render_sharded refuses two contexts of one device whose states differ in one part, naming that part's setter.

The triangles are media_scenes' `area` (an area light, an interface box, an opaque quad: 28 triangles) with
lights_scenes' spot added, so that every stop has a light.  While the context holds media the scene has no
medium of its own; without them the same triangles stand in one homogeneous fog, and after the media are
cleared in the 8^3 grid medium, so that the scene's own medium record is walked as well.

The walk runs once (a module fixture keeps what the context returned at each stop); the restatement is the
slow side, a second or two per stop, so each stop is a case of its own.
"""
import functools

import numpy as np
import pytest

import lights_scenes as ls
import media_scenes as ms

pytestmark = pytest.mark.gpu

N_PHOTONS, MAX_DEPTH, RADIUS = 300, 5, 0.01
W = H = 16
BEAM_KEYS = ("start", "end", "radius", "power")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def build_state():
    import importlib

    sm = importlib.import_module("beam-radiance-estimate-pbrt_amd.scene")
    meshes, _, fog, _ = ms.meshes_of("area")
    spot = sm.spot_light(ls.SPOT_FROM, ls.SPOT_TO, ls.SPOT_I, 30.0, 5.0, 0)
    bare = sm.make_scene(meshes)
    fogged = sm.make_scene(meshes, 0.05, 0.5, 0.0)
    gridded = sm.grid_medium(sm.make_scene(meshes, 0.5, 4.5, 0.7), ls.grid_density8(), 8)
    materials, tri_mat = sm.scene_materials(meshes)
    media = sm.scene_media(meshes, fog, [fog])
    # a different table of the same sizes: other coefficients, a coloured sigma_s, forward and backward g
    other = [sm.medium_homogeneous(0.1, 0.8, 0.4), sm.medium_homogeneous((0.3, 0.2, 0.1), (1.0, 1.5, 2.0), -0.3)]
    assert len(other) == len(media[0]) and bare.n_triangles == 28
    assert any(m.type == sm.MATERIAL_INTERFACE for m in materials)
    return bare, fogged, gridded, [spot], materials, tri_mat, media, (other,) + tuple(media[1:])


def stops():
    """The walk: (name, the setter call that leads there, then the state: scene, lights, materials, map, media
    (None or set_media's five arguments), and the iteration both passes run at).  The iterations are ones at
    which the restatement's surface radiance is not all zero."""
    bare, fogged, gridded, lights, materials, tri_mat, media, media2 = build_state()
    return [("1 no state", None, fogged, [], [], [], None, 0),
            ("2 lights", lambda g: g.set_lights(lights), fogged, lights, [], [], None, 3),
            ("3 media", lambda g: g.set_media(*media), bare, lights, [], [], media, 0),
            ("4 materials", lambda g: g.set_materials(materials, tri_mat), bare, lights, materials, tri_mat, media, 2),
            ("5 media replaced", lambda g: g.set_media(*media2), bare, lights, materials, tri_mat, media2, 2),
            ("6 materials cleared", lambda g: g.set_materials(), bare, lights, [], [], media2, 3),
            ("7 media cleared", lambda g: g.set_media(), gridded, lights, [], [], None, 1),
            ("8 lights cleared", lambda g: g.set_lights(), gridded, [], [], [], None, 3)]


N_STOPS = 8


@pytest.fixture(scope="module")
def walked(bre):
    """Per stop what the one context returned: (beam count, beams, segment count, segments, surface)."""
    import torch

    out = []
    with bre.BeamGather(0) as g:
        for _, setter, scene, _, _, _, _, iteration in stops():
            if setter:
                setter(g)
            nb = g.trace_photons(scene, N_PHOTONS, iteration, MAX_DEPTH, RADIUS)
            beams = g.get_beams()
            surf = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
            ns = g.camera_pass(scene, W, H, iteration, MAX_DEPTH, surface=surf)
            seg = g.get_segments()
            torch.cuda.synchronize()
            out.append((nb, beams, ns, seg, surf.cpu().numpy()))
    assert len(out) == N_STOPS
    return out


@functools.lru_cache(maxsize=None)
def restatement(stop):
    """Both passes of the state at `stop`, computed once per session (tests/test_refpy_golden.py pins them too)."""
    import refpy_passes as rpass

    scene, lights, materials, tri_mat, media, iteration = stops()[stop][2:]
    assert media is not None or not materials  # an interface entry never outlives the media
    sc = rpass.Scene(scene, lights, materials, tri_mat, *(media or ()))
    return (rpass.trace_photons(sc, N_PHOTONS, iteration, MAX_DEPTH, RADIUS),
            rpass.camera_pass(sc, W, H, iteration, MAX_DEPTH))


def sorted_segments(seg):
    order = np.lexsort((seg["depth"], seg["pixel"]))
    return {k: seg[k][order] for k in ("o", "p", "d", "tmax", "pixel", "depth")}


@pytest.mark.parametrize("stop", range(N_STOPS))
def test_walk_stop_equals_its_restatement(walked, stop):
    what = stops()[stop][0]
    ref_beams, ref_cam = restatement(stop)
    nb, beams, ns, seg, surf = walked[stop]
    assert nb == int(ref_beams["counts"].sum()) and nb > 0, what
    for k in BEAM_KEYS:
        assert np.array_equal(bits(beams[k]), bits(ref_beams[k])), (what, k)
    assert ns == seg["o"].shape[0] == ref_cam["o"].shape[0] and ns > 0, what
    a, r = sorted_segments(seg), sorted_segments(ref_cam)
    assert np.array_equal(a["pixel"], r["pixel"]) and np.array_equal(a["depth"], r["depth"]), what
    for k in ("o", "p", "d", "tmax"):
        assert np.array_equal(bits(a[k]), bits(r[k])), (what, k)
    assert ref_cam["surface"].max() > 0, what
    assert np.array_equal(bits(surf), bits(ref_cam["surface"])), what


def test_render_sharded_names_the_part_that_differs(bre, scene_mod_gpu):
    sm = scene_mod_gpu
    bare, _, _, lights, materials, tri_mat, media, media2 = build_state()
    p = sm.render_params(W, H, iterations=1, photons=N_PHOTONS, max_depth=MAX_DEPTH, radius=0.05, alpha=0.5)
    dimmer = [sm.spot_light(ls.SPOT_FROM, ls.SPOT_TO, (6.0, 6.0, 6.0), 30.0, 5.0, 0)]
    one_matte = list(tri_mat)
    one_matte[tri_mat.index(max(tri_mat))] = -1  # one interface triangle back to its own kd
    with bre.BeamGather(0) as a, bre.BeamGather(0) as b:
        for g in (a, b):
            g.set_lights(lights)
            g.set_media(*media)
            g.set_materials(materials, tri_mat)
        for change, restore, setter in ((lambda: b.set_lights(dimmer), lambda: b.set_lights(lights), "bre_set_lights"),
                                        (lambda: b.set_media(*media2), lambda: b.set_media(*media), "bre_set_media"),
                                        (lambda: b.set_materials(materials, one_matte),
                                         lambda: b.set_materials(materials, tri_mat), "bre_set_materials")):
            change()
            with pytest.raises(bre.BreError) as e:
                bre.render_sharded([a, b], bare, p)
            msg = str(e.value)
            assert e.value.status == 1 and "context 1" in msg and f"({setter}) differ from context 0's" in msg, msg
            assert sum(s in msg for s in ("bre_set_lights", "bre_set_media", "bre_set_materials")) == 1, msg
            restore()
