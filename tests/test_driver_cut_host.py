"""The host's cut rules for FASTQ input (thermite_amd/csrc/fastq_cut.h): tests/cpp/driver_cut_main.cpp checks the cut of a
block that is not the last, the cut of a mapped plain file and the grouping of BGZF members against naive restatements,
exhaustively over small inputs.  The header compiles without the HIP runtime; the program is built as
test_extend_plan_host builds its own, plain and under the host sanitizers, and run directly."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_program(tmp_dir, sanitizers=False):
    exe = os.path.join(str(tmp_dir), "driver_cut_main" + ("_san" if sanitizers else ""))
    extra = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if sanitizers else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra +
                          ["-I" + os.path.join(ROOT, "thermite_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "driver_cut_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("sanitizers", [False, True], ids=["plain", "sanitizers"])
def test_cut_rules_against_naive_restatements(sanitizers, tmp_path):
    r = subprocess.run([host_program(tmp_path, sanitizers)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    m = re.fullmatch(r"cases (\d+)\n", r.stdout)
    # 8191 strings over {'a', '\n'} of length 0 to 12: one block cut each; every start x 8 line counts x 4 span sizes (1, 3,
    # 8 and the default) for the mapped cut, 32 x 98305; 13 sizes x every start of the 1092 member vectors, 13 x 6015
    assert m and int(m.group(1)) >= 8191 + 32 * 98305 + 13 * 6015, r.stdout
