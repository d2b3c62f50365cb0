"""Compile-time resources of the tier-3 photon and camera kernels (k_photons_mx<MODE, MED>, k_camera_mx<MED>: the walk
of tier 2 over the wide lobe lists of a table that holds a mix), by the mechanism of tests/test_frosted_resources.py.
No GPU is needed; skipped where hipcc is absent.

* The new kernels spill no VGPR and hold at least 2 waves per SIMD (their __launch_bounds__, kMixWaves).
* Their VGPRs and scratch are pinned at what the compiler reports for the code as it stands.
* The kernels of tiers 0 to 2 are held by tests/test_glossy_resources.py and tests/test_frosted_resources.py, unedited.
"""
import pytest

from test_glossy_resources import _one, _unit

# (VGPRs, scratch bytes per lane, waves per SIMD); keys (mode, med) and med
PINNED_PHOTONS_MX = {(0, 0): (128, 0, 4), (0, 1): (128, 0, 4), (1, 0): (128, 0, 4), (1, 1): (128, 0, 4),
                     (2, 0): (136, 0, 3), (2, 1): (136, 0, 3)}
PINNED_CAMERA_MX = {0: (155, 0, 3), 1: (172, 0, 2)}


@pytest.fixture(scope="module")
def photon_remarks(tmp_path_factory):
    return _unit(tmp_path_factory, "bre_photon")


@pytest.fixture(scope="module")
def camera_remarks(tmp_path_factory):
    return _unit(tmp_path_factory, "bre_camera")


def _row(r):
    return (r["VGPRs"], r["ScratchSize [bytes/lane]"], r["Occupancy [waves/SIMD]"])


def test_photon_kernels_of_tier_3(photon_remarks):
    rows = {key: _one(photon_remarks, f"k_photons_mxILi{key[0]}ELb{key[1]}EE") for key in PINNED_PHOTONS_MX}
    for (mode, med), r in rows.items():
        print(f"k_photons_mx<{mode}, {med}>", _row(r), r["VGPRs Spill"], r["SGPRs Spill"])
    for key, r in rows.items():
        assert r["VGPRs Spill"] == 0 and r["Occupancy [waves/SIMD]"] >= 2, (key, r)
        assert _row(r) == PINNED_PHOTONS_MX[key], key


def test_camera_kernels_of_tier_3(camera_remarks):
    rows = {med: _one(camera_remarks, f"k_camera_mxILb{med}EE") for med in PINNED_CAMERA_MX}
    for med, r in rows.items():
        print(f"k_camera_mx<{med}>", _row(r), r["VGPRs Spill"], r["SGPRs Spill"])
    for med, r in rows.items():
        assert r["VGPRs Spill"] == 0 and r["Occupancy [waves/SIMD]"] >= 2, (med, r)
        assert _row(r) == PINNED_CAMERA_MX[med], med
