"""Media bounded by surfaces without a GPU: the restatement (tests/refpy_passes.py) with a media table of one
against the scene's own medium, hand-derived known answers of the pass-through, the condition that the scenes of
the GPU tests reach every branch, and the Python view of the media."""
import ctypes
import importlib

import numpy as np
import pytest

import media_scenes as ms
import pass_refs
import refpy_media as rm
import refpy_passes as rpass
import specular_scenes as ss
from refpy_photon import RNG, expf, offset_origin

f32 = np.float32


@pytest.fixture(scope="module")
def sm():
    return importlib.import_module("beam-radiance-estimate-pbrt_amd.scene")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------- a table of one, no transition anywhere, is the scene's own medium ----------------
@pytest.mark.parametrize("name", ["prism", "grid"])
def test_one_entry_table_equals_the_specular_restatement(sm, name):
    scene, lights, mats, tri_mat = ss.build(name)
    n = scene.n_triangles
    if scene.has_medium == sm.MEDIUM_GRID:
        cells = scene.grid_n[0] * scene.grid_n[1] * scene.grid_n[2]
        dens = np.ctypeslib.as_array((ctypes.c_float * cells).from_address(scene.grid_density)).copy()
        medium = sm.medium_grid(tuple(scene.sigma_a), tuple(scene.sigma_s), scene.g, dens, tuple(scene.grid_n),
                                np.array(list(scene.world_to_medium), np.float32).reshape(4, 4))
    else:
        medium = sm.medium_homogeneous(tuple(scene.sigma_a), tuple(scene.sigma_s), scene.g)
    bare = type(scene).from_buffer_copy(scene)
    bare.has_medium = sm.MEDIUM_NONE
    media = ([medium], [0] * n, [0] * n, 0, [0] * len(lights))
    own, tabled = rpass.Scene(scene, lights, mats, tri_mat), rpass.Scene(bare, lights, mats, tri_mat, *media)
    for it in (0, 2):
        want = rpass.trace_photons(own, 150, it, 5, 0.01)
        stats = rpass.new_stats()
        got = rpass.trace_photons(tabled, 150, it, 5, 0.01, stats=stats)
        assert np.array_equal(got["counts"], want["counts"]) and want["counts"].sum() > 100
        for k in ("start", "end", "radius", "power"):
            assert np.array_equal(bits(got[k]), bits(want[k])), (name, it, k)
        assert not any(stats[k] for k in rpass.MEDIA_COUNTERS)
    want = rpass.camera_pass(own, 10, 10, 1, 4)
    got = rpass.camera_pass(tabled, 10, 10, 1, 4)
    for k in ("o", "p", "d", "tmax", "surface"):
        assert np.array_equal(bits(got[k]), bits(want[k])), (name, k)
    assert np.array_equal(got["pixel"], want["pixel"]) and np.array_equal(got["depth"], want["depth"])
    assert want["surface"].max() > 0 and want["o"].shape[0] >= 100


# ---------------- hand-derived known answers: a slab between two interface quads ----------------
SIGMA = (0.2, 0.3)  # sigma_a, sigma_s: sigma_t = 0.5
X0, X1 = 0.3, 0.6
LE = (5.0, 3.0, 2.0)


def quad_x(x, kd, Le, material, pair):
    """A quad in the plane x = const spanning the unit square, with the right Cornell wall's winding (normal -x)."""
    return ([(x, 0, 0), (x, 0, 1), (x, 1, 1), (x, 1, 0)], (0, 1, 2, 0, 2, 3), kd, Le, material, pair)


def slab_case(sm):
    """Vacuum, an interface at x = 0.3, the medium up to the interface at x = 0.6, vacuum, a black emitting wall at 1."""
    face = sm.interface()
    med = sm.medium_homogeneous(SIGMA[0], SIGMA[1], 0.0)
    # the normals point to -x: `outside` is the -x side
    meshes = [quad_x(X0, ss.UNUSED_KD, None, face, (med, None)), quad_x(X1, ss.UNUSED_KD, None, face, (None, med)),
              quad_x(1.0, (0, 0, 0), LE, None, None)]
    scene = sm.make_scene(meshes, cam_pos=(0.02, 0.5, 0.4), cam_look=(1.0, 0.5, 0.4), cam_up=(0.0, 1.0, 0.0),
                          fov=20.0)
    mats, tri_mat = sm.scene_materials(meshes)
    return (scene, [], mats, tri_mat) + tuple(sm.scene_media(meshes))


def test_photon_through_a_slab_makes_three_beams(sm):
    case = slab_case(sm)
    sc = rpass.Scene(*case)
    assert all(t["n"] == (f32(-1), f32(0), f32(0)) for t in sc.tris) and sc.iface == [True] * 4 + [False] * 2
    o, d = (f32(0), f32(0.5), f32(0.25)), (f32(1), f32(0), f32(0))
    beta = (f32(2), f32(3), f32(4))
    sigma_t = f32(f32(SIGMA[0]) + f32(SIGMA[1]))
    # the three hits and the slab segment's length L', found one ray at a time
    h1, _ = sc.intersect(o, d)
    o2 = offset_origin(h1[0], h1[1], sc.tris[h1[2]]["n"], d)
    h2, L = sc.intersect(o2, d)  # |d| = 1: tMax is the offset-origin-to-hit length
    o3 = offset_origin(h2[0], h2[1], sc.tris[h2[2]]["n"], d)
    h3, _ = sc.intersect(o3, d)
    assert (h1[2] // 2, h2[2] // 2, h3[2] // 2) == (0, 1, 2)
    assert o2[0] > h1[0][0] and o3[0] > h2[0][0] and abs(float(L) - (X1 - X0)) < 1e-6
    seq = next(s for s in range(1, 50) if rm.med_sample(sc.media[0], RNG(s), o2, d, L) is None)  # no scattering event
    stats = rpass.new_stats()
    rng, out = RNG(seq), []
    rpass.walk(sc, rng, out, o, d, 0, beta, -1, 5, 0.01, stats)
    assert len(out) == 3 and stats["photon_pass"] == 2 and stats["vacuum_segment"] == 2
    assert [b[0] for b in out] == [o, o2, o3] and [b[1] for b in out] == [h1[0], h2[0], h3[0]]
    tr = expf(f32(f32(-sigma_t) * L))
    assert 0.85 < tr < 0.87  # exp(-0.15)
    # the un-attenuated beta is carried through the slab: the third beam has the first one's power
    assert out[0][3] == beta and out[1][3] == tuple(f32(tr * b) for b in beta) and out[2][3] == beta
    # draws: the slab's Sample (2), then the Get2D at the black wall (2); none at the two quads
    fresh = RNG(seq)
    for _ in range(4):
        fresh.uniform()
    assert rng.uniform() == fresh.uniform()


def test_camera_path_through_a_slab_has_three_segments_at_depth_zero(sm):
    case = slab_case(sm)
    stats = rpass.new_stats()
    out = rpass.camera_pass(rpass.Scene(*case), 1, 1, 0, 1, stats=stats)  # maxdepth 1: everything happens at depth 0
    assert out["o"].shape[0] == 3 and list(out["depth"]) == [0, 1, 2] and list(out["pixel"]) == [0, 0, 0]
    assert stats["camera_pass"] == 2 and stats["vacuum_segment"] == 2 and stats["camera_pass_roulette"] == 0
    assert np.allclose(out["p"][:, 0], [X0, X1, 1.0], atol=1e-6) and (out["o"][1:, 0] > out["p"][:-1, 0]).all()
    # isect.Le at depth 0 with beta = Tr of the slab, once: |d| * tMax of the middle segment is its length
    d = tuple(f32(x) for x in out["d"][1])
    sigma_t = f32(f32(SIGMA[0]) + f32(SIGMA[1]))
    x = f32(f32(out["tmax"][1]) * f32(np.sqrt(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2])))))
    tr = expf(f32(f32(-sigma_t) * x))
    assert X1 - X0 - 1e-6 <= float(x) <= (X1 - X0) / np.cos(np.radians(15.0))  # the pixel's ray is oblique
    assert np.array_equal(bits(out["surface"][0]), bits(np.array([f32(tr * f32(v)) for v in LE], np.float32)))
    # with rendersurfaces off the path still passes through the interfaces and ends at the first BSDF
    off = rpass.camera_pass(rpass.Scene(*case), 1, 1, 0, 1, render_surfaces=False)
    assert off["o"].shape[0] == 3 and not off["surface"].any()


# ---------------- the scenes of the GPU tests reach every branch ----------------
def test_gpu_scenes_take_every_branch_at_least_20_times():
    total = rpass.new_stats()
    over = {}
    for name in ms.NAMES:
        assert ms.build(name).scene.n_triangles <= 60
        for it in ms.PHOTON_ITERATIONS:
            for k, v in pass_refs.photon_ref(ms, name, it)[1].items():
                total[k] += v
        for it in ms.CAMERA_ITERATIONS:
            ref, stats = pass_refs.camera_ref(ms, name, it)
            for k, v in stats.items():
                total[k] += v
            over[name, it] = int((np.bincount(ref["pixel"]) > ms.CAM_DEPTH).sum())
    for k in rpass.MEDIA_COUNTERS:
        assert total[k] >= 20, (k, total)
    # pixels whose path records more segments than maxdepth: the camera pass needs its segment budget
    assert all(over[name, it] > 0 for name in ("box", "camera_in") for it in ms.CAMERA_ITERATIONS), over


# ---------------- the Python view ----------------
def test_python_view_of_the_media(sm):
    bre = importlib.import_module("beam-radiance-estimate-pbrt_amd")
    assert "bre_set_media" in bre.EXPORTS and bre.OPT_SEGMENT_BUDGET == 17
    assert ctypes.sizeof(sm.Medium) == 120 and sm.Medium.grid_density.offset == 112  # no padding: bre_medium
    assert sm.interface().type == sm.MATERIAL_INTERFACE == 3 and sm.MAX_MEDIA == 64
    a, b = sm.medium_homogeneous(0.1, (1, 2, 3), 0.5), sm.medium_grid(1.0, 2.0, -0.2, np.ones(24), (2, 3, 4))
    assert (a.type, b.type) == (sm.MEDIUM_HOMOGENEOUS, sm.MEDIUM_GRID)
    assert tuple(a.sigma_s) == (1, 2, 3) and tuple(b.grid_n) == (2, 3, 4) and b.grid_density
    quad = ([(0, 0, 0), (0, 0, 1), (1, 0, 1), (1, 0, 0)], sm.QUAD, sm.WHITE, None)
    meshes = [quad, quad + (sm.interface(), (b, None)), quad + (None, (a, b)), quad + (None, None)]
    media, ti, to, cm, lm = sm.scene_media(meshes, a, [None, b])
    assert [m.type for m in media] == [b.type, a.type]  # in order of first use
    assert ti == [-1, -1, 0, 0, 1, 1, -1, -1] and to == [-1, -1, -1, -1, 0, 0, -1, -1] and cm == 1 and lm == [-1, 0]
    assert sm.make_scene(meshes).n_triangles == 8
    lib = bre.load_library()
    assert lib.bre_set_media(None, None, 0, None, None, 0, -1, None, 0) == 1  # no context


# ---------------- the .pbrt front end ----------------
@pytest.fixture(scope="module")
def pb():
    return importlib.import_module("beam-radiance-estimate-pbrt_amd.pbrt")


HEAD = ('LookAt 0.5 0.5 0.02  0.5 0.5 1  0 1 0\nCamera "perspective" "float fov" [60]\n'
        'Film "image" "integer xresolution" [16] "integer yresolution" [16]\nIntegrator "photonbeam"\nWorldBegin\n')
FOG = 'MakeNamedMedium "fog" "string type" "homogeneous" "rgb sigma_a" [0.05 0.05 0.05] "rgb sigma_s" [0.5 0.5 0.5]\n'
SMOKE = 'MakeNamedMedium "smoke" "string type" "homogeneous" "rgb sigma_a" [1 1 1] "rgb sigma_s" [8 8 8] "float g" [0.2]\n'
SPOT = 'LightSource "spot" "point from" [0.5 0.9 0.5] "point to" [0.5 0 0.5]\n'
FLOOR = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0 0 0  0 0 1  1 0 1  1 0 0]\n'
QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0.2 0.5 0.2  0.2 0.5 0.8  0.8 0.5 0.8  0.8 0.5 0.2]\n'


def test_parser_accepts_media_only_with_the_flag(pb, sm):
    # a medium transition on a wall
    text = HEAD + FOG + SPOT + 'MediumInterface "" "fog"\n' + FLOOR + "WorldEnd\n"
    s = pb.parse_string(text)
    assert not s.ok and "one medium" in s.messages
    s = pb.parse_string(text, media=True)
    assert s.ok and s.n_errors == 0, s.messages
    assert s.scene.has_medium == sm.MEDIUM_NONE and len(s.media) == 1 and s.media[0].type == sm.MEDIUM_HOMOGENEOUS
    assert tuple(s.media[0].sigma_s) == (0.5, 0.5, 0.5) and list(s.tri_inside) == [-1, -1] and list(s.tri_outside) == [0, 0]
    assert s.camera_medium == 0 and list(s.light_medium) == [-1] and not s.materials
    # a shape without a material: skipped with an error by default, an interface triangle with the flag
    text = (HEAD + SMOKE + SPOT + FLOOR + 'AttributeBegin\nMaterial "none"\nMediumInterface "smoke" ""\n' + QUAD +
            "AttributeEnd\nWorldEnd\n")
    s = pb.parse_string(text)
    assert s.n_errors == 1 and "shapes without a material (medium boundaries) are not supported" in s.messages
    s = pb.parse_string(text, media=True)
    assert s.ok and s.n_errors == 0, s.messages
    assert [m.type for m in s.materials] == [sm.MATERIAL_INTERFACE] and list(s.triangle_material) == [-1, -1, 0, 0]
    assert list(s.tri_inside) == [-1, -1, 0, 0] and list(s.tri_outside) == [-1] * 4 and s.camera_medium == -1
    assert s.media[0].g == np.float32(0.2) and tuple(s.media[0].sigma_a) == (1, 1, 1)
    # the empty name is the same material
    s = pb.parse_string(text.replace('Material "none"', 'Material ""'), media=True)
    assert s.ok and [m.type for m in s.materials] == [sm.MATERIAL_INTERFACE]
    # a light declared in another medium than the camera's
    text = HEAD + FOG + SPOT + 'MediumInterface "fog" "fog"\n' + FLOOR + "WorldEnd\n"
    s = pb.parse_string(text)
    assert not s.ok and "light 0 is declared in medium" in s.messages
    s = pb.parse_string(text, media=True)
    assert s.ok and list(s.light_medium) == [-1] and s.camera_medium == 0
    assert list(s.tri_inside) == [0, 0] and list(s.tri_outside) == [0, 0]
    # equal media share one entry, others get their own; only media in use are listed
    twin = FOG.replace('"fog"', '"mist"')
    text = (HEAD + FOG + twin + SMOKE + SPOT + 'MediumInterface "fog" "mist"\n' + FLOOR + 'MediumInterface "fog" ""\n' +
            QUAD + "WorldEnd\n")
    s = pb.parse_string(text, media=True)
    assert s.ok and len(s.media) == 1 and list(s.tri_outside) == [0, 0, -1, -1] and list(s.tri_inside) == [0] * 4
    s = pb.parse_string(text.replace('"fog" "mist"\n', '"fog" "smoke"\n'), media=True)
    assert s.ok and len(s.media) == 2 and list(s.tri_outside) == [1, 1, -1, -1]
    # an undefined medium is pbrt's error with the flag too
    text = HEAD + FOG + SPOT + 'MediumInterface "nope" ""\n' + FLOOR + "WorldEnd\n"
    assert not pb.parse_string(text).ok
    s = pb.parse_string(text, media=True)
    assert not s.ok and 'Named medium "nope" undefined.' in s.messages
    # a boundary around nothing
    s = pb.parse_string(HEAD + SPOT + FLOOR + 'Material "none"\n' + QUAD + "WorldEnd\n", media=True)
    assert not s.ok and "bound no medium" in s.messages


def test_smoke_box_scene_file(pb, sm):
    import os

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes", "smoke_box.pbrt")
    s = pb.parse_file(path)
    assert s.n_errors >= 1 and "medium boundaries" in s.messages  # it needs the flag
    s = pb.parse_file(path, media=True)
    assert s.ok and s.n_errors == 0 and s.n_warnings == 0, s.messages
    assert s.scene.n_triangles == 36 and s.scene.has_medium == sm.MEDIUM_NONE and len(s.lights) == 1
    assert [m.type for m in s.media] == [sm.MEDIUM_HOMOGENEOUS] * 2 and tuple(s.media[1].sigma_s) == (12, 18, 24)
    assert [m.type for m in s.materials] == [sm.MATERIAL_INTERFACE, sm.MATERIAL_GLASS]
    assert list(s.triangle_material) == [-1] * 12 + [0] * 12 + [1] * 12
    assert list(s.tri_inside) == [-1] * 12 + [0] * 12 + [1] * 12 and list(s.tri_outside) == [-1] * 36
    assert s.camera_medium == -1 and list(s.light_medium) == [-1]
    # the boxes are specular_scenes.box_mesh's: the hand-built scene has the file's triangles
    meshes = ([m + (None,) for m in sm.cornell_meshes()[:-1]] +
              [ss.box_mesh((0.3, 0.25, 0.45), (0.5, 0.5, 0.65), sm.interface()),
               ss.box_mesh((0.56, 0.25, 0.55), (0.72, 0.45, 0.71), sm.glass(1.0, 1.0, 1.5))])
    hand = sm.make_scene(meshes)
    for i in range(36):
        assert bytes(hand.triangles[i].p) == bytes(s.scene.triangles[i].p), i
