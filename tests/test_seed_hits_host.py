"""CPU side of the per-hit entry points (thm_extend_left_right_batch, thm_align_seed_hits_batch): exports, struct
layouts and the C++ mirror's methods.  No compute calls: there is no GPU in the CPU test run."""
import ctypes
import os
import subprocess

from thermite_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_per_hit_symbols_exported():
    L = ctypes.CDLL(capi.SO_PATH)
    for s in ("thm_extend_left_right_batch", "thm_align_seed_hits_batch"):
        assert s in capi.ABI_SYMBOLS
        assert hasattr(L, s), "missing export: " + s


def _c_sizeof(tmp_path, exprs):
    src = tmp_path / "sz.c"
    body = "".join('  printf("%%zu\\n", (size_t)(%s));\n' % e for e in exprs)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "thermite.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return [int(v) for v in subprocess.check_output([str(exe)]).split()]


def test_per_hit_struct_layouts_match_header(tmp_path):
    lr_fields = ["ystart", "yend", "ylen", "ops_off", "score", "xstart", "xend", "xlen", "ops_len"]
    exprs = ["sizeof(thm_lr_aln)"] + ["offsetof(thm_lr_aln, %s)" % f for f in lr_fields]
    exprs += ["sizeof(thm_lr_view)", "sizeof(thm_hits_view)", "offsetof(thm_hits_view, n_failed_hits)",
              "offsetof(thm_hits_view, hit_status)", "sizeof(thm_aln)", "sizeof(thm_mem)"]
    got = _c_sizeof(tmp_path, exprs)
    assert got[0] == capi.LR_DT.itemsize == 56
    assert got[1:10] == [capi.LR_DT.fields[f][1] for f in lr_fields]
    assert got[10] == ctypes.sizeof(capi.LrView)
    assert got[11] == ctypes.sizeof(capi.HitsView)
    assert got[12] == capi.HitsView.n_failed_hits.offset and got[13] == capi.HitsView.hit_status.offset
    assert got[14] == capi.ALN_DT.itemsize and got[15] == capi.MEM_DT.itemsize


def test_cpp_driver_compiles_against_mirror_header(tmp_path):
    """tests/cpp/seed_hits_main.cpp calls Aligner::extend_left_right and Aligner::align_seed_hits (compile and link only)"""
    exe = tmp_path / "seed_hits_main"
    libdir = os.path.dirname(capi.SO_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "seed_hits_main.cpp"), "-o", str(exe), "-L" + libdir,
                           "-lthermite_amd", "-Wl,-rpath," + libdir])
    assert exe.exists()
