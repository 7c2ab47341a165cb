"""CPU side of the device BGZF encoder (include/thermite_io.h: thm_bgzf_view and the calls around it): the ABI, and the
encoder's steps (thermite_amd/csrc/bgzf_device.h, the functions kernels_bgzf.hip spreads over threads) run serially on
the host by tests/cpp/bgzf_model_main.cpp over the edge cases of tests/test_gpu_bgzf.py."""
import ctypes
import os
import re
import subprocess

import pytest

import bgzf_common as zc
from thermite_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["thm_batch_fetch_bgzf", "thm_align_batch_bgzf"]


def test_abi_symbols_and_view_layout(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "thermite_io.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in capi.IO_ABI_SYMBOLS
        assert hasattr(capi.lib(), s), "missing export: " + s
    assert hasattr(capi.lib(), "thm_debug_bgzf_device") and "thm_debug_bgzf_device" not in hdr
    core = open(os.path.join(ROOT, "include", "thermite.h")).read()
    assert "THM_T_BGZF = 7" in core and "THM_N_TIMINGS = 8" in core
    assert capi.TIMING_NAMES[7] == "bgzf" and len(capi.TIMING_NAMES) == capi.N_TIMINGS == 8
    assert "THM_BAM_DEVICE=2" in hdr
    # the C compiler's layout of thm_bgzf_view against the ctypes structure
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "thermite_io.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(thm_bgzf_view));\n' +
                   "".join('  printf(" %%zu", offsetof(thm_bgzf_view, %s));\n' % f for f, _ in capi.BgzfView._fields_) +
                   '  printf(" %d %d\\n", (int)THM_T_BGZF, (int)THM_N_TIMINGS);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True).stdout.split()]
    want = [ctypes.sizeof(capi.BgzfView)] + [getattr(capi.BgzfView, f).offset for f, _ in capi.BgzfView._fields_] + [7, 8]
    assert got == want and ctypes.sizeof(capi.BgzfView) == 72
    assert [f for f, _ in capi.BgzfView._fields_] == ["n_reads", "n_records", "n_raw_bytes", "n_blocks", "n_bytes", "data", "block_off",
                                                      "n_failed_reads", "read_status"]


def test_cpp_header_has_the_bgzf_call(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "thermite.hpp"\nauto p1 = &thermite::Aligner::align_reads_bgzf;\n'
                   "thermite::Aligner::BgzfBlocks b;\nint main() { return (int)b.block_off.size(); }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "bgzf_main.cpp")])


def test_null_arguments_need_no_device():
    L = capi.lib()
    v = capi.BgzfView()
    assert L.thm_batch_fetch_bgzf(None, 0, ctypes.byref(v)) == capi.ERR_INVALID_ARG
    assert L.thm_align_batch_bgzf(None, None, 0, ctypes.byref(v)) == capi.ERR_INVALID_ARG
    assert L.thm_align_batch_bgzf(None, None, 0, None) == capi.ERR_INVALID_ARG
    n = ctypes.c_uint64(0)
    assert L.thm_debug_bgzf_device(None, None, 0, None, 0, ctypes.byref(n), ctypes.byref(n)) == capi.ERR_INVALID_ARG


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bgzf_model") / "bgzf_model_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "thermite_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "bgzf_model_main.cpp"), "-o", str(exe)])
    return exe


def test_the_encoder_steps_on_the_host(model, tmp_path):
    """every edge case through the serial run of the kernel's steps: each member passes check_blocks and the stream
    inflates to the input; incompressible input comes back stored and within n + 5 + 26 a member; a run of one byte and
    a repeated motif use matches (far below the literal-only size)"""
    for name, raw in zc.edge_cases().items():
        (tmp_path / "in.bin").write_bytes(raw)
        subprocess.check_call([str(model), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
        got, payload, stored = zc.check_blocks((tmp_path / "out.bin").read_bytes())
        assert got == raw, name
        assert len(payload) == -(-len(raw) // zc.BLOCK_IN), name
        if name == "random":
            assert all(stored) and all(p <= zc.BLOCK_IN + 5 for p in payload)
        if name in ("zeros", "motif_200", "period_1019"):
            assert sum(payload) < len(raw) // 30 and not any(stored), name
        if name == "de_bruijn_4_4":   # no match, 259 literals of two bits and the header
            assert not stored[0] and payload[0] < 120
        if name == "twice_32768":   # the second copy is found at a distance of exactly 32768: the block costs the random
            assert payload[0] < 32768 * 21 // 20 + 1024   # half as literals of a little over 8 bits, and the copy next to nothing
        if name == "twice_32769":   # ... and 32769 is out of the window
            assert payload[0] >= zc.BLOCK_IN
