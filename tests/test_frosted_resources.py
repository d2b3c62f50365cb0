"""Compile-time resources of the photon and camera kernels after the tier with the BSDF of any number of lobes
(k_photons_tr<MODE, MED>, k_camera_tr<MED>; rough glass, uber, translucent, substrate), by the mechanism of
tests/test_glossy_resources.py.  No GPU is needed; skipped where hipcc is absent.

* The new kernels have zero scratch, spill no VGPR and hold at least 2 waves per SIMD (their __launch_bounds__).
* The walk is now one body shared by the three tiers (photon_walk, camera_walk).  The <..., true> instantiations are
  no worse than the resource table of DESIGN.md section 25 (commit c4a0da5), copied below: no more VGPRs, zero
  scratch, no lower occupancy.
* The <..., false> ones are no worse than tests/test_glossy_resources.py's parent constants.
"""
import pytest

from test_glossy_resources import PARENT_CAMERA, PARENT_PHOTONS, _camera, _no_worse, _one, _photons, _unit

# (VGPRs, scratch bytes per lane, waves per SIMD) of the <..., true> instantiations at commit c4a0da5 (DESIGN.md
# section 25, "Kernel resources"); keys (mode, med) and med
C4A0DA5_PHOTONS_TRUE = {(1, 1): (112, 0, 4), (1, 0): (111, 0, 4), (2, 1): (114, 0, 4), (2, 0): (114, 0, 4),
                        (0, 1): (111, 0, 4), (0, 0): (111, 0, 4)}
C4A0DA5_CAMERA_TRUE = {1: (170, 0, 2), 0: (125, 0, 4)}


@pytest.fixture(scope="module")
def photon_remarks(tmp_path_factory):
    return _unit(tmp_path_factory, "bre_photon")


@pytest.fixture(scope="module")
def camera_remarks(tmp_path_factory):
    return _unit(tmp_path_factory, "bre_camera")


def _new_kernels(photon_remarks, camera_remarks):
    out = {f"k_photons_tr<{mode}, {med}>": _one(photon_remarks, f"k_photons_trILi{mode}ELb{med}EE")
           for mode in (0, 1, 2) for med in (0, 1)}
    out.update({f"k_camera_tr<{med}>": _one(camera_remarks, f"k_camera_trILb{med}EE") for med in (0, 1)})
    return out


def test_new_kernels_have_zero_scratch_no_spill_two_waves(photon_remarks, camera_remarks):
    kernels = _new_kernels(photon_remarks, camera_remarks)
    for name, r in kernels.items():
        print(name, {k: r[k] for k in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
                                       "VGPRs Spill", "SGPRs Spill")})
    for name, r in kernels.items():
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r["ScratchSize [bytes/lane]"])
        assert r["VGPRs Spill"] == 0 and r["Occupancy [waves/SIMD]"] >= 2, (name, r)


def test_glossy_instantiations_no_worse_than_c4a0da5(photon_remarks, camera_remarks):
    for (mode, med), parent in C4A0DA5_PHOTONS_TRUE.items():
        r = _photons(photon_remarks, mode, med, True)
        print(f"k_photons<{mode}, {med}, true>", r["VGPRs"], r["ScratchSize [bytes/lane]"], r["Occupancy [waves/SIMD]"])
        _no_worse(r, parent)
    for med, parent in C4A0DA5_CAMERA_TRUE.items():
        r = _camera(camera_remarks, med, True)
        print(f"k_camera<{med}, true>", r["VGPRs"], r["ScratchSize [bytes/lane]"], r["Occupancy [waves/SIMD]"])
        _no_worse(r, parent)


def test_plain_instantiations_no_worse_than_parent_constants(photon_remarks, camera_remarks):
    for (mode, med), parent in PARENT_PHOTONS.items():
        r = _photons(photon_remarks, mode, med, False)
        print(f"k_photons<{mode}, {med}, false>", r["VGPRs"], r["ScratchSize [bytes/lane]"], r["Occupancy [waves/SIMD]"])
        _no_worse(r, parent)
    for med, parent in PARENT_CAMERA.items():
        r = _camera(camera_remarks, med, False)
        print(f"k_camera<{med}, false>", r["VGPRs"], r["ScratchSize [bytes/lane]"], r["Occupancy [waves/SIMD]"])
        _no_worse(r, parent)
