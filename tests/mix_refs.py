"""The references of the mix pass tests (test infrastructure): tests/refpy_passes_mix.py on scene `name` of
tests/mix_scenes.py at that module's sizes, each computed once per (scene, iteration) and shared by every test of the
session, CPU and GPU; the returned arrays are not to be modified.
"""
import functools

import mix_scenes as ms
import refpy_passes_mix as rpm


@functools.lru_cache(maxsize=None)
def scene(name):
    return rpm.Scene(*ms.build(name))


@functools.lru_cache(maxsize=None)
def photon_ref(name, iteration):
    """(beams, per-beam tags, stats)."""
    sc, stats = scene(name), rpm.new_stats()
    ref, tags = rpm.trace_photons(sc, ms.N_PHOTONS, iteration, ms.MAX_DEPTH, ms.RADIUS, stats=stats)
    return ref, tags, stats


DEEP_PHOTONS = 200


@functools.lru_cache(maxsize=None)
def deep_photon_ref(name, max_depth):
    """The beams of the first DEEP_PHOTONS photons of iteration 0 at `max_depth`."""
    ref, _ = rpm.trace_photons(scene(name), DEEP_PHOTONS, 0, max_depth, ms.RADIUS)
    return ref


@functools.lru_cache(maxsize=None)
def camera_ref(name, iteration):
    """(segments and surface radiance, info, stats)."""
    sc, stats = scene(name), rpm.new_stats()
    ref, info = rpm.camera_pass(sc, ms.CAM_W, ms.CAM_H, iteration, ms.CAM_DEPTH, stats=stats)
    return ref, info, stats
