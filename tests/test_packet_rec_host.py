"""csrc/bre_packet.h on the host (CPU): the packet records' sizing and indexing.  tests/packet_rec_check.cpp
includes the header alone (it has no HIP include), is built with the host compiler under AddressSanitizer and
UBSan and run as a child process: for gathers of one launch and of several (internal option 109), whole and
ragged last packets and a packet shard's renumbered segments, every record a tile wave reads must be one its own
launch wrote, inside a buffer sized by the launch's packet count."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("packet_rec") / "packet_rec_check")
    # the sanitizer runtimes are linked statically: the program needs nothing preloaded
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "beam-radiance-estimate-pbrt_amd", "csrc"),
                    os.path.join(ROOT, "tests", "packet_rec_check.cpp"), "-o", exe], check=True)
    return exe


def test_packet_records_sizing_and_indexing(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "0 failures", r.stdout + r.stderr
