"""The extend stage's launch plan (thermite_amd/csrc/extend_plan.h) on the host: tests/cpp/extend_plan_main.cpp evaluates
the plan over a grid of read lengths, bands, batch sizes, CU counts, coordinate widths and launch mixes, asserts the
invariants of the counter-row layout, the trace slices and the grids at every point, and pins the values of a few
shapes derived by hand.  The header compiles without the HIP runtime; the program is built as smem_finish_common.host_program
builds its own, plain and under the host sanitizers, and run directly."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_program(tmp_dir, sanitizers=False):
    exe = os.path.join(str(tmp_dir), "extend_plan_main" + ("_san" if sanitizers else ""))
    extra = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if sanitizers else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra +
                          ["-I" + os.path.join(ROOT, "thermite_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "extend_plan_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("sanitizers", [False, True], ids=["plain", "sanitizers"])
def test_plan_invariants_and_anchors(sanitizers, tmp_path):
    r = subprocess.run([host_program(tmp_path, sanitizers)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    m = re.fullmatch(r"points (\d+) checks (\d+)\n", r.stdout)
    # 8 lengths x the bands a length can have, by score and by fraction, x retries x batch sizes (alone / mixed) x 3 CU
    # counts x 2 widths x 4 paths (the usual one, three DP kernel sizes of the
    # problem-parallel one) x 2 finisher settings: the grid does not shrink unnoticed
    assert m and int(m.group(1)) >= 60000 and int(m.group(2)) > 30 * int(m.group(1)), r.stdout

