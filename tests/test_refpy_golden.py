"""The pure-Python restatement of the two passes (tests/refpy_passes.py) against the outputs of the layered
restatements it replaced, recorded at the commit named in tests/golden/refpy_parent.json: per case the shape,
dtype and SHA-256 of every returned array and the branch counters the producing layer kept.  The restatement
is the expected value of every bit-exact GPU test of the passes, so nothing here is tolerated or skipped.

The cases are the GPU tests' own (their scenes, sizes and iterations, read from the scene modules), the eight
stops of tests/test_scene_state_gpu.py and the pins of tests/test_photon_oracle.py and tests/test_lights_refpy.py;
each goes through the cache its test uses, so no reference is computed twice in a session.  `pin/photon` stands
for the former test that the light layer without delta lights was the photon layer.

Scene.intersect filters its candidates; the last test holds it to the exhaustive loop on whole passes.
"""
import hashlib
import importlib
import json
import os

import numpy as np
import pytest

import lights_scenes as ls
import media_scenes as ms
import pass_refs
import refpy_passes as rpass
import specular_scenes as ss
import test_lights_refpy as tlr
import test_photon_oracle as tpo
import test_scene_state_gpu as tss

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refpy_parent.json")))
CASES = GOLDEN["cases"]
MODULES = {"lights": ls, "specular": ss, "media": ms}
PIN_NAMES, PIN_ITERATIONS = ("fog", "grid"), (0, 3)


def expected_ids():
    ids = []
    for tag, mod in MODULES.items():
        photon = getattr(mod, "PHOTON_NAMES", mod.NAMES)
        camera = getattr(mod, "CAMERA_NAMES", mod.NAMES)
        ids += [f"{tag}/photon/{n}/{it}" for n in photon for it in mod.PHOTON_ITERATIONS]
        ids += [f"{tag}/camera/{n}/{it}" for n in camera for it in mod.CAMERA_ITERATIONS]
    ids += [f"state/{i}/{what}" for i in range(tss.N_STOPS) for what in ("photon", "camera")]
    ids += [f"oracle/fog/{i}" for i in range(len(tpo.FOG_CASES))] + [f"oracle/grid/{i}" for i in range(len(tpo.GRID_CASES))]
    ids += [f"pin/photon/{n}" for n in PIN_NAMES] + [f"pin/camera/{n}/{it}" for n in PIN_NAMES for it in PIN_ITERATIONS]
    return ids


def recompute(case):
    """(arrays, stats or None) of a case, through the cache of the test that uses it."""
    part = case.split("/")
    if part[0] in MODULES:
        ref = pass_refs.photon_ref if part[1] == "photon" else pass_refs.camera_ref
        return ref(MODULES[part[0]], part[2], int(part[3]))
    if part[0] == "state":
        return tss.restatement(int(part[1]))[part[2] == "camera"], None
    if part[0] == "oracle":
        return tpo.restated(part[1], int(part[2]))[1], None
    if part[1] == "camera":
        return tlr.pin_camera(part[2], int(part[3]))[1], None
    sm = importlib.import_module("beam-radiance-estimate-pbrt_amd.scene")
    return rpass.trace_photons(rpass.Scene(tlr.pin_scenes(sm)[part[2]]), 200, 1, 5, 0.01), None


def test_the_golden_file_holds_exactly_the_cases_of_the_tests():
    assert sorted(CASES) == sorted(expected_ids())
    assert len(GOLDEN["parent"]) == 40 and all(c["producer"] for c in CASES.values())


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_equals_the_recorded_parent(case):
    want = CASES[case]
    got, stats = recompute(case)
    for k, w in want["arrays"].items():
        a = np.ascontiguousarray(got[k])
        assert list(a.shape) == w["shape"] and str(a.dtype) == w["dtype"], (case, k, a.shape, a.dtype)
        assert hashlib.sha256(a.tobytes()).hexdigest() == w["sha256"], (case, k)
    if "stats" in want:  # the counters the producing layer kept; the single restatement keeps all of COUNTERS
        assert {k: stats[k] for k in want["stats"]} == want["stats"], case


@pytest.mark.parametrize("mod,name", [(ss, "prism"), (ss, "grid"), (ms, "nested"), (ms, "area")],
                         ids=["specular-prism", "specular-grid", "media-nested", "media-area"])
def test_filtered_intersect_equals_the_exhaustive_one_on_whole_passes(mod, name):
    state = mod.build(name)
    filtered, exhaustive = rpass.Scene(*state), rpass.Scene(*state, exhaustive=True)
    assert not filtered.exhaustive and exhaustive.exhaustive
    for it in (0, 2):
        a, b = (rpass.trace_photons(sc, 150, it, 5, 0.01) for sc in (filtered, exhaustive))
        assert a["counts"].sum() > 100
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), (name, it, k)
    a, b = (rpass.camera_pass(sc, 10, 10, 1, 4) for sc in (filtered, exhaustive))
    assert a["o"].shape[0] >= 100
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (name, k)
