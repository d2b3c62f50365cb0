"""The references of the bit-exact pass tests (test infrastructure): tests/refpy_passes.py on scene `name` of a
scene module (lights_scenes, specular_scenes, media_scenes) at that module's sizes.

The restatement is the slow side (seconds per pass): each reference is computed once per (module, scene,
iteration) and shared by every test of the session, CPU and GPU; the returned arrays are not to be modified.
"""
import functools

import refpy_passes as rpass


@functools.lru_cache(maxsize=None)
def scene(mod, name):
    return rpass.Scene(*mod.build(name))


@functools.lru_cache(maxsize=None)
def photon_ref(mod, name, iteration):
    """(beams, stats); beams["infos"] holds trace_photon's info per photon."""
    stats, infos = rpass.new_stats(), []
    ref = rpass.trace_photons(scene(mod, name), mod.N_PHOTONS, iteration, mod.MAX_DEPTH, mod.RADIUS, infos=infos,
                              stats=stats)
    ref["infos"] = infos
    return ref, stats


@functools.lru_cache(maxsize=None)
def camera_ref(mod, name, iteration):
    """(segments and surface radiance, stats)."""
    stats = rpass.new_stats()
    ref = rpass.camera_pass(scene(mod, name), mod.CAM_W, mod.CAM_H, iteration, mod.CAM_DEPTH, stats=stats)
    return ref, stats
