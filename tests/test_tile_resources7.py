"""Compile-time resources of the tile kernel's seven-wave specialised instantiation.

k_gather_tile<false, 7, TileProd> (bre_gather.hip, internal option 124 = 7) exists to put seven waves on
every SIMD without a spill: 72 allocated VGPRs give seven waves where 80 give six, and 28 one-wave
workgroups per CU fit its 160 KB of LDS only at 5,851 B each or less.  The gather unit is compiled once
for the device only, with the Makefile's own `isa` target (its flags,
-Rpass-analysis=kernel-resource-usage), and the remark lines must say for the seven-wave instantiation: at
most 72 VGPRs, occupancy 7, no scratch, no SGPR spill, at most 5,851 B of LDS; and for the six-wave one
what tests/test_tile_resources.py asks of it, within the same LDS.  Only the remarks are read, not the
assembly.  No GPU is needed; skipped where hipcc is absent."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beam-radiance-estimate-pbrt_amd", "csrc")
LDS_PER_CU = 163840  # bytes; 4 SIMDs x 7 waves = 28 one-wave workgroups must fit


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def _remarks(text):
    """{mangled kernel name: {remark key: int}} from the kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        body = m.group(1)
        f = re.match(r"Function Name:\s*(\S+)", body)
        if f:
            cur = out.setdefault(f.group(1), {})
            continue
        kv = re.match(r"(.+?):\s*(-?\d+)\s*$", body)
        if kv and cur is not None:
            cur[kv.group(1).strip()] = int(kv.group(2))
    return out


@pytest.fixture(scope="module")
def tile_remarks(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    obj = tmp_path_factory.mktemp("tile_isa7")
    subprocess.run(["make", "-C", CSRC, "isa", "UNIT=bre_gather", f"OBJDIR={obj}", f"HIPCC={hipcc}"], check=True,
                   stdout=subprocess.DEVNULL)
    with open(os.path.join(obj, "isa", "resource_usage.txt")) as fh:
        return _remarks(fh.read())


def _tile(remarks, count, minw, fixed):
    """The remarks of k_gather_tile<count, minw, TileCfg<fixed>> (Itanium mangling of the template arguments)."""
    tag = f"k_gather_tileILb{int(count)}ELi{minw}ENS0_7TileCfgILb{int(fixed)}EEEE"
    hits = [v for k, v in remarks.items() if tag in k]
    assert len(hits) == 1, (tag, sorted(remarks))
    return hits[0]


def test_seven_wave_instantiation_fits_without_spills(tile_remarks):
    r = _tile(tile_remarks, False, 7, True)
    print("k_gather_tile<false, 7, TileProd>:", r)
    assert r["VGPRs"] <= 72
    assert r["Occupancy [waves/SIMD]"] == 7
    assert r["ScratchSize [bytes/lane]"] == 0
    assert r["SGPRs Spill"] == 0
    assert r["VGPRs Spill"] == 0
    assert r["LDS Size [bytes/block]"] <= LDS_PER_CU // 28 == 5851


def test_six_wave_instantiation_keeps_its_figures(tile_remarks):
    r = _tile(tile_remarks, False, 6, True)
    print("k_gather_tile<false, 6, TileProd>:", r)
    assert r["VGPRs"] <= 80
    assert r["Occupancy [waves/SIMD]"] == 6
    assert r["SGPRs Spill"] == 0
    assert r["ScratchSize [bytes/lane]"] == 0
    assert r["LDS Size [bytes/block]"] <= LDS_PER_CU // 28
