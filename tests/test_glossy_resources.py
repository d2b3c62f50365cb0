"""Compile-time resources of the photon and camera kernels, by the mechanism of tests/test_tile_resources.py: each unit
is compiled once for the device only with the Makefile's own `isa` target, and only the kernel-resource-usage remarks
are read.  No GPU is needed; skipped where hipcc is absent.

* The instantiations that existed before the glossy materials (k_photons<MODE, MED, false>, k_camera<MED, false>) run
  inside another context's gather: VGPRs, scratch and occupancy no worse than at the parent
  commit 1e65dfe ("Specialise the production tile kernel on its launch constants"), whose numbers are the constants
  below (compiled from that commit with the same target).
* The glossy instantiations (<..., true>) have zero scratch and spill no VGPR.  The photon walk's stack of suspended
  frames, a per-thread array in the other instantiations (their 1216-1296 bytes per lane), lives in the block's dynamic
  LDS there (csrc/bre_photon.hip), and the camera kernel inlines estimate_direct at its one call, which as a call
  took the sampler through memory.
"""
import os
import subprocess

import pytest

from test_tile_resources import CSRC, _hipcc, _remarks

# (VGPRs, scratch bytes per lane, waves per SIMD) at the parent commit 1e65dfe
PARENT_PHOTONS = {(0, 0): (80, 1216, 6), (0, 1): (80, 1296, 6), (1, 0): (80, 1216, 6), (1, 1): (80, 1296, 6),
                  (2, 0): (80, 1232, 6), (2, 1): (80, 1296, 6)}
PARENT_CAMERA = {0: (80, 140, 6), 1: (80, 300, 6)}


def _unit(tmp_path_factory, unit):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    obj = tmp_path_factory.mktemp(unit + "_isa")
    subprocess.run(["make", "-C", CSRC, "isa", f"UNIT={unit}", f"OBJDIR={obj}", f"HIPCC={hipcc}"], check=True,
                   stdout=subprocess.DEVNULL)
    with open(os.path.join(obj, "isa", "resource_usage.txt")) as fh:
        return _remarks(fh.read())


@pytest.fixture(scope="module")
def photon_remarks(tmp_path_factory):
    return _unit(tmp_path_factory, "bre_photon")


@pytest.fixture(scope="module")
def camera_remarks(tmp_path_factory):
    return _unit(tmp_path_factory, "bre_camera")


def _one(remarks, tag):
    hits = [v for k, v in remarks.items() if tag in k]
    assert len(hits) == 1, (tag, sorted(remarks))
    return hits[0]


def _photons(remarks, mode, med, glossy):
    return _one(remarks, f"k_photonsILi{mode}ELb{med}ELb{int(glossy)}EE")


def _camera(remarks, med, glossy):
    return _one(remarks, f"k_cameraILb{med}ELb{int(glossy)}EE")


def _no_worse(r, parent):
    vgprs, scratch, waves = parent
    assert r["VGPRs"] <= vgprs and r["ScratchSize [bytes/lane]"] <= scratch and r["Occupancy [waves/SIMD]"] >= waves, r


def test_existing_photon_instantiations_no_worse_than_parent(photon_remarks):
    for (mode, med), parent in PARENT_PHOTONS.items():
        _no_worse(_photons(photon_remarks, mode, med, False), parent)


def test_existing_camera_instantiations_no_worse_than_parent(camera_remarks):
    for med, parent in PARENT_CAMERA.items():
        _no_worse(_camera(camera_remarks, med, False), parent)


def _glossy(photon_remarks, camera_remarks):
    out = {f"k_photons<{mode}, {med}, true>": _photons(photon_remarks, mode, med, True)
           for mode in (0, 1, 2) for med in (0, 1)}
    out.update({f"k_camera<{med}, true>": _camera(camera_remarks, med, True) for med in (0, 1)})
    return out


def test_glossy_instantiations_have_zero_scratch(photon_remarks, camera_remarks):
    for name, r in _glossy(photon_remarks, camera_remarks).items():
        print(name, {k: r[k] for k in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill")})
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r["ScratchSize [bytes/lane]"])
        assert r["VGPRs Spill"] == 0 and r["Occupancy [waves/SIMD]"] >= 2, (name, r)
