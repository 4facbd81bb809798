"""The scratch helper of the launch functions on the host (no GPU): parallel-gps_amd/csrc/pgps_scratch.h -- the bump carver
every launch function lays its device scratch out with, and batch_group, the one rule by which B items run in groups that fit
a scratch budget -- compiled with g++ into a stand-alone program (tests/cpu_math/scratch.cpp) and run.  The carver is checked
over 10 000 seeded random sequences of parts (empty parts, 4- / 8- / 16-byte elements, 128- and 256-byte alignment: aligned
offsets, disjoint parts, the last part inside bytes(), an empty part at its successor's offset, and every offset equal to the
hand-written `off = up(off + n * sizeof(T))` form it replaces); batch_group against the literal formula on a table of edges.
One build also runs under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {"O2": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("flags", list(FLAGS), ids=list(FLAGS))
def test_carver_and_batch_group(flags, tmp_path):
    exe = str(tmp_path / "scratch")
    subprocess.run(["g++"] + FLAGS[flags] + ["-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "parallel-gps_amd", "csrc"),
                                             os.path.join(ROOT, "tests", "cpu_math", "scratch.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.strip().endswith("scratch ok")
    assert "carver: 10000 sequences" in run.stdout
