"""Compile-time resources of the tile kernel's specialised production instantiation.

k_gather_tile<false, 6, TileProd> (bre_gather.hip) exists to run without register spills: the generic
instantiation carries its options in SGPRs, spills 18 of them to lanes of a reserved VGPR and keeps
16 B per lane of scratch.  The gather unit is compiled once for the device only, with the Makefile's
own `isa` target (its flags, -Rpass-analysis=kernel-resource-usage), and the remark lines of the
specialised instantiation must say: at most 80 VGPRs, occupancy 6, no SGPR spill, no scratch.  Only
the remarks are read, not the assembly.  No GPU is needed; skipped where hipcc is absent."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "beam-radiance-estimate-pbrt_amd", "csrc")


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
    obj = tmp_path_factory.mktemp("tile_isa")
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


def test_specialised_instantiation_has_no_spills(tile_remarks):
    r = _tile(tile_remarks, False, 6, True)
    print("k_gather_tile<false, 6, TileProd>:", r)
    assert r["VGPRs"] <= 80
    assert r["Occupancy [waves/SIMD]"] == 6
    assert r["SGPRs Spill"] == 0
    assert r["ScratchSize [bytes/lane]"] == 0


def test_generic_instantiation_is_still_built(tile_remarks):
    """Every other setting (and option 123 = 0) runs the generic instantiation at the same occupancy."""
    r = _tile(tile_remarks, False, 6, False)
    assert r["Occupancy [waves/SIMD]"] == 6
