"""CPU: the host image and the device block layout behind PathPlanner's candidate calls
(csrc/candidate_batch.h: CandidateLayout), compiled with AddressSanitizer and
UndefinedBehaviorSanitizer into a small stand-alone program (tests/candidate_layout_host.cpp)
that lays out the parts of every candidate call and checks them: every part 256-byte aligned,
no two overlapping, all inside the block; the offsets, waypoints and segment ranges of the
ragged sets."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(cxx):
        cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("candlayout") / "candidate_layout_host")
    cc = subprocess.run([cxx, "-x", "c++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(ROOT, "include"),
                         os.path.join(ROOT, "tests", "candidate_layout_host.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, f"compiling tests/candidate_layout_host.cpp with {cxx} failed:\n{cc.stderr}"
    return exe


def _lines(host, gates, sizes):
    run = subprocess.run([host, str(gates)] + [str(w) for w in sizes], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines
    return lines


# one single-segment set; it beside a longer one, either way round (part sizes that are no
# multiples of 256 bytes); 32 sets (the offsets and statuses fill 256 bytes and more: n + 1 = 33
# int32, n = 32 int64 exactly 256); a batch whose times pass one 256-byte line
RAGGED = [(2,), (2, 17), (17, 2), (2, 2, 2), (3, 31, 2, 9, 12), tuple(2 + (7 * k) % 30 for k in range(32)),
          tuple(2 + (5 * k) % 11 for k in range(33)), (2,) * 64, (34, 2)]


@pytest.mark.parametrize("sizes", RAGGED, ids=lambda s: f"n{len(s)}w{sum(s)}")
@pytest.mark.parametrize("gates", [0, 1, 8, 64])
def test_parts_are_aligned_apart_and_inside(host, gates, sizes):
    lines = _lines(host, gates, sizes)
    image = lines[0].split()
    n, total = len(sizes), sum(sizes)
    assert image[:7] == ["image", "n", str(n), "total", str(total), "nseg", str(total - n)]
    assert int(image[8]) % 256 == 0
    # at least the shared parts, each rounded up to 256 bytes
    up = lambda b: (b + 255) // 256 * 256
    assert int(image[8]) == up(24 * total) + up(8 * (total - n)) + up(240 * (total - n)) + up(4 * (n + 1)) + up(4 * n)
    checks = [ln for ln in lines[1:]]
    assert len(checks) == 5 + 3 * 11 and all(ln.endswith(" ok") for ln in checks), checks


@pytest.mark.parametrize("sizes", [(1,), (5, 1), (0, 4), (2, 3, 1)])
def test_a_short_set_throws_before_the_layout(host, sizes):
    assert _lines(host, 4, sizes) == ["short ok"]
