"""The control rule of the in-kernel mode search and the scratch layout of pgps_gp_panel_laplace_* on the host (no GPU):
parallel-gps_amd/csrc/pgps_newton.h -- the accept / halve / converge functions and newton_search, the loop k_gpp_newton runs
per workgroup -- and pgps_panel_site_lay.h, compiled with g++ into a stand-alone program (tests/cpu_math/newton_ctl.cpp) and
run.  The program drives the SAME functions over scalar toy problems (one Poisson count under a wide prior, where undamped
Newton overflows; one Bernoulli observation), checks termination within the caps for NaN and infinite Psi and moves, and
checks the layout of 2000 seeded random panels (groups within the budget, slices aligned, disjoint and inside their parts).
One build also runs under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = {"O2": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("flags", list(FLAGS), ids=list(FLAGS))
def test_newton_control_and_scratch_layout(flags, tmp_path):
    exe = str(tmp_path / "newton_ctl")
    subprocess.run(["g++"] + FLAGS[flags] + ["-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "parallel-gps_amd", "csrc"),
                                             os.path.join(ROOT, "tests", "cpu_math", "newton_ctl.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout + run.stderr)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.strip().endswith("newton ok")
    assert "layout: 2000 panels" in run.stdout
