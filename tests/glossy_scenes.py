"""The scenes of the plastic / metal / Oren-Nayar tests (test infrastructure): name -> media_scenes.Case (scene, lights,
materials, triangle_material and the media arguments, empty where the scene has its own fog).  Every scene has at
most 40 triangles.

plastic  the Cornell walls in fog, the floor and the back wall of plastic (one with the defaults' remapped roughness,
         one with alpha 0.3 given directly), a point light
metal    the walls in fog, the oblique spot of spot_fog.pbrt, an anisotropic metal box (alphas 0.05 and 0.4) in the
         spot's shaft and a near-mirror metal quad (alpha 0.001) on the floor beside it
rough    Oren-Nayar walls (sigma 20, and 90 on the side walls) under the Cornell area light: both MIS halves of
         EstimateDirect run with a BSDF::Pdf that is the cosine's but an f that is not
mixed    plastic floor, metal and mirror quads, an interface box of smoke and a glass box holding a grid medium, in
         thin fog (bre_set_media)
onelobe  a plastic with Ks 0, one with Kd 0, a matte entry with sigma 0 and a plastic with both black (no BxDF)
glossy_fog     (not in NAMES) scenes/glossy_fog.pbrt built by hand: a plastic floor, Oren-Nayar walls, a metal plate
onelobe_plain  (not in NAMES) onelobe with the Ks-0 plastic and the sigma-0 matte entry as the triangles' own kd
"""
import functools
import importlib

import lights_scenes as ls
from media_scenes import Case, boundary, unit_cube_to
from specular_scenes import BOX_HI, BOX_LO, UNUSED_KD, box_mesh, floor_mirror_quad

NAMES = ("plastic", "metal", "rough", "mixed", "onelobe")
N_PHOTONS, MAX_DEPTH, RADIUS = 2000, 5, 0.01
PHOTON_ITERATIONS, CAMERA_ITERATIONS = (0, 2), (0, 3)
CAM_W = CAM_H = 24
CAM_DEPTH = 5
COPPER_ETA, COPPER_K = (0.2004, 0.9240, 1.1022), (3.9129, 2.4528, 2.1421)  # an RGB stand-in for the copper spectra
ONELOBE_KD = (0.73, 0.73, 0.73)


def _sm():
    return importlib.import_module("beam-radiance-estimate-pbrt_amd.scene")


def _with(mesh, material):
    return mesh[:3] + (mesh[3], material) + tuple(mesh[5:])


def meshes_of(name):
    """(meshes with material and medium pair, fog arguments or None, lights, camera medium, light media)."""
    sm = _sm()
    walls = [m + (None, None) for m in sm.cornell_meshes()[:-1]]  # floor, ceiling, back, front, left, right
    spot = sm.spot_light(ls.SPOT_FROM, ls.SPOT_TO, ls.SPOT_I, 30.0, 5.0, 0)
    point = sm.point_light(ls.POINT_P, ls.POINT_I)
    fog = (0.05, 0.5, 0.0)
    if name == "plastic":
        walls[0] = _with(walls[0], sm.plastic((0.4, 0.3, 0.2), 0.5, 0.1, True))
        walls[2] = _with(walls[2], sm.plastic(0.25, 0.25, 0.3, False))
        return walls, fog, [point], None, []
    if name == "metal":
        box = box_mesh(BOX_LO, BOX_HI, sm.metal(COPPER_ETA, COPPER_K, 0.01, 0.05, 0.4, False))
        quad = floor_mirror_quad(sm.metal(COPPER_ETA, COPPER_K, 0.001, remap=False))
        return walls + [box, quad], fog, [spot], None, []
    if name == "rough":
        light = sm.cornell_meshes()[-1] + (None, None)
        for k, sigma in ((0, 20.0), (1, 20.0), (2, 20.0), (4, 90.0), (5, 90.0)):
            walls[k] = _with(walls[k], sm.matte(walls[k][2], sigma))
        return walls + [light], fog, [], None, []
    if name == "mixed":
        thin = sm.medium_homogeneous(0.05, 0.5, 0.0)
        smoke = sm.medium_homogeneous(1.0, 8.0, 0.0)
        glo, ghi = (0.12, 0.05, 0.35), (0.32, 0.25, 0.55)
        grid = sm.medium_grid(1.0, 9.0, 0.7, ls.grid_density8(), 8, unit_cube_to(glo, ghi))
        walls[0] = _with(walls[0], sm.plastic((0.5, 0.5, 0.5), 0.3, 0.1, True))
        smoke_box = boundary(box_mesh(BOX_LO, BOX_HI, sm.interface()), smoke, thin)
        glass_box = boundary(box_mesh(glo, ghi, sm.glass(1.0, 1.0, 1.5)), grid, thin)
        mirror = floor_mirror_quad(sm.mirror(0.9)) + (None,)
        metal = ([(0.6, 0.3, 0.995), (0.6, 0.7, 0.995), (0.95, 0.7, 0.995), (0.95, 0.3, 0.995)], (0, 1, 2, 0, 2, 3),
                 UNUSED_KD, None, sm.metal(COPPER_ETA, COPPER_K, 0.2, remap=False), None)
        return walls + [smoke_box, glass_box, mirror, metal], None, [spot], thin, [thin]
    if name == "glossy_fog":  # scenes/glossy_fog.pbrt built by hand, in the file's order
        white = sm.matte(sm.WHITE, 20.0)
        walls[0] = _with(walls[0][:2] + (UNUSED_KD,) + walls[0][3:], sm.plastic(0.5, 0.25, 0.1, True))
        for k in (1, 2, 3):
            walls[k] = _with(walls[k], white)
        walls[4] = _with(walls[4], sm.matte(sm.RED, 20.0))
        walls[5] = _with(walls[5], sm.matte(sm.GREEN, 20.0))
        plate = floor_mirror_quad(sm.metal(COPPER_ETA, COPPER_K, 0.05))
        return walls + [plate], fog, [spot], None, []
    if name in ("onelobe", "onelobe_plain"):
        plain = name == "onelobe_plain"
        if plain:
            walls[0] = walls[0][:2] + (ONELOBE_KD,) + walls[0][3:]
        else:
            walls[0] = _with(walls[0], sm.plastic(ONELOBE_KD, 0.0, 0.1, True))
            walls[4] = _with(walls[4], sm.matte(walls[4][2], 0.0))
        walls[2] = _with(walls[2], sm.plastic(0.0, 0.6, 0.2, False))
        walls[5] = _with(walls[5], sm.plastic(0.0, 0.0, 0.1, True))
        return walls, fog, [point], None, []
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def build(name):
    sm = _sm()
    meshes, fog, lights, cam_med, light_media = meshes_of(name)
    scene = sm.make_scene(meshes, *fog) if fog else sm.make_scene(meshes)
    materials, tri_mat = sm.scene_materials(meshes)
    if cam_med is None and not any(len(m) > 5 and m[5] is not None for m in meshes):
        media, ti, to, cm, lm = [], [], [], -1, []
    else:
        media, ti, to, cm, lm = sm.scene_media(meshes, cam_med, light_media)
    assert scene.n_triangles <= 40
    return Case(scene, lights, materials, tri_mat, media, ti, to, cm, lm)


def apply(g, case):
    """Put the case's lights, media and materials on context `g` (the media first: an interface needs them)."""
    g.set_lights(case.lights)
    g.set_media(case.media, case.tri_inside, case.tri_outside, case.camera_medium, case.light_medium)
    g.set_materials(case.materials, case.tri_mat)
