"""The references of the plastic / metal / Oren-Nayar pass tests (test infrastructure): tests/refpy_passes_bsdf.py on
scene `name` of tests/glossy_scenes.py at that module's sizes, each computed once per (scene, iteration) and shared
by every test of the session, CPU and GPU; the returned arrays are not to be modified.
"""
import functools

import glossy_scenes as gs
import refpy_passes_bsdf as rpb


@functools.lru_cache(maxsize=None)
def scene(name):
    return rpb.Scene(*gs.build(name))


@functools.lru_cache(maxsize=None)
def photon_ref(name, iteration):
    """(beams, stats, the (r, phi) of the pass's normal-incidence microfacet samples)."""
    sc, stats = scene(name), rpb.new_stats()
    first = len(sc.normals)
    ref = rpb.trace_photons(sc, gs.N_PHOTONS, iteration, gs.MAX_DEPTH, gs.RADIUS, stats=stats)
    return ref, stats, tuple(sc.normals[first:])


DEEP_PHOTONS = 300


@functools.lru_cache(maxsize=None)
def deep_photon_ref(name, max_depth):
    """(beams, the normal-incidence samples) of the first DEEP_PHOTONS photons of iteration 0 at `max_depth`."""
    sc = scene(name)
    first = len(sc.normals)
    ref = rpb.trace_photons(sc, DEEP_PHOTONS, 0, max_depth, gs.RADIUS)
    return ref, tuple(sc.normals[first:])


@functools.lru_cache(maxsize=None)
def camera_ref(name, iteration):
    """(segments and surface radiance, stats, the normal-incidence samples)."""
    sc, stats = scene(name), rpb.new_stats()
    first = len(sc.normals)
    ref = rpb.camera_pass(sc, gs.CAM_W, gs.CAM_H, iteration, gs.CAM_DEPTH, stats=stats)
    return ref, stats, tuple(sc.normals[first:])
