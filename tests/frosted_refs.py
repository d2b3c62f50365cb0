"""The references of the rough glass / uber / translucent / substrate pass tests (test infrastructure):
tests/refpy_passes_full.py on scene `name` of tests/frosted_scenes.py at that module's sizes, each computed once per
(scene, iteration) and shared by every test of the session, CPU and GPU; the returned arrays are not to be modified.
"""
import functools

import frosted_scenes as fs
import refpy_passes_full as rpf


@functools.lru_cache(maxsize=None)
def scene(name):
    return rpf.Scene(*fs.build(name))


@functools.lru_cache(maxsize=None)
def photon_ref(name, iteration):
    """(beams, per-beam tags, stats, the (r, phi) of the pass's normal-incidence microfacet samples)."""
    sc, stats = scene(name), rpf.new_stats()
    first = len(sc.normals)
    ref, tags = rpf.trace_photons(sc, fs.N_PHOTONS, iteration, fs.MAX_DEPTH, fs.RADIUS, stats=stats)
    return ref, tags, stats, tuple(sc.normals[first:])


DEEP_PHOTONS = 200


@functools.lru_cache(maxsize=None)
def deep_photon_ref(name, max_depth):
    """(beams, the normal-incidence samples) of the first DEEP_PHOTONS photons of iteration 0 at `max_depth`."""
    sc = scene(name)
    first = len(sc.normals)
    ref, _ = rpf.trace_photons(sc, DEEP_PHOTONS, 0, max_depth, fs.RADIUS)
    return ref, tuple(sc.normals[first:])


@functools.lru_cache(maxsize=None)
def camera_ref(name, iteration):
    """(segments and surface radiance, info, stats, the normal-incidence samples)."""
    sc, stats = scene(name), rpf.new_stats()
    first = len(sc.normals)
    ref, info = rpf.camera_pass(sc, fs.CAM_W, fs.CAM_H, iteration, fs.CAM_DEPTH, stats=stats)
    return ref, info, stats, tuple(sc.normals[first:])
