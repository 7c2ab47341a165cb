"""The host-only parts of thermite_amd/csrc/run_summary.h under AddressSanitizer and UBSan, without a device:
tests/cpp/run_summary_main.cpp is built as a stand-alone program (its own main, nothing preloaded) and fed every shape
view and every bad view of tests/cov_common.py and tests/pileup_common.py, written out the way the model programs'
inputs are.  A shape must pass the checks of thm_coverage_add_view / thm_pileup_add_view, a bad view must be refused
with THM_ERR_INVALID_ARG and a message that names alignment 1; the layout's arithmetic is checked by the program itself.

    python tools/run_summary_host_check.py [work_dir]

Prints what the program printed and "ok", or raises."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cov_common as cv  # noqa: E402
import pileup_common as pc  # noqa: E402
from thermite_amd import capi  # noqa: E402

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
WANT = {"past_the_contig": "lies beyond the", "no_refid": "has no @SQ line", "outside_the_pool": "are outside the pool", "query_length": "its M + I + S is"}


def build(work):
    exe = os.path.join(work, "run_summary_main")
    csrc = os.path.join(ROOT, "thermite_amd", "csrc")
    subprocess.check_call([os.path.join(ROCM, "lib", "llvm", "bin", "clang++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
                           "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROCM, "include"),
                           os.path.join(ROOT, "tests", "cpp", "run_summary_main.cpp"),
                           "-L" + os.path.join(ROCM, "lib"), "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-lamdhip64", "-lpthread", "-o", exe])
    return exe


def run(exe, mode, t, data):
    p = subprocess.run([exe, mode, str(len(t["txs"])), str(len(t["genes"]))], input=data, capture_output=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    sys.stdout.write(p.stdout.decode())
    if p.returncode != 0:
        raise SystemExit("%s: exit %d\n%s" % (mode, p.returncode, p.stderr.decode()))
    return [line.split(" ", 3) for line in p.stdout.decode().splitlines() if line.startswith("view ")]


def check(exe, mode, t, model_input, shapes, bad):
    good = [v for name in sorted(shapes) for v in shapes[name]]
    lines = run(exe, mode, t, model_input(t, 0, good + [bad[name] for name in sorted(bad)]))
    assert len(lines) == len(good) + len(bad), (mode, len(lines))
    for k, line in enumerate(lines[:len(good)]):
        assert line[2] == "0", (mode, "shape view", k, line)
    for name, line in zip(sorted(bad), lines[len(good):]):
        assert int(line[2]) == capi.ERR_INVALID_ARG and "alignment 1" in line[3] and WANT[name] in line[3], (mode, name, line)
    print("%s: %d shape views pass, %d bad views refused" % (mode, len(good), len(bad)))


def main():
    work = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="run_summary_")
    os.makedirs(work, exist_ok=True)
    exe = build(work)
    t = cv.shape_tables()
    check(exe, "cov", t, cv.model_input, cv.shape_cases(t, capi.COV_TILE), cv.bad_views(t))
    t = pc.shape_tables()
    shapes = pc.shape_cases(t, capi.PILE_CHUNK, capi.PILE_GROUP, capi.COV_TILE)
    check(exe, "pile", t, pc.model_input, shapes, pc.bad_views(t))
    print("ok")


if __name__ == "__main__":
    main()
