"""CPU side of the device FASTQ parser (include/thermite_io.h: thm_batch_upload_fastq, thm_batch_fetch_reads): the ABI,
and the parser's steps (thermite_amd/csrc/fastq_device.h, the functions kernels_fastq.hip spreads over threads) run
serially on the host by tests/cpp/fastq_model_main.cpp over the blocks of tests/test_gpu_fastq_device.py, against the
host block parser (fastq_parse_block, through FastqReader.all_by_blocks)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fastq_device_common as fc
from thermite_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["thm_batch_upload_fastq", "thm_batch_fetch_reads"]
_WELL, _DECLINED = fc.well_formed(), fc.declined()


def test_abi_symbols_and_info_layout(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "thermite_io.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in capi.IO_ABI_SYMBOLS
        assert hasattr(capi.lib(), s), "missing export: " + s
    assert set(re.findall(r"\b(thm_[a-z0-9_]+)\s*\(", hdr)) == set(capi.IO_ABI_SYMBOLS)
    assert hasattr(capi.lib(), "thm_debug_fastq_device_blocks") and "thm_debug_fastq_device_blocks" not in hdr
    assert "THM_FASTQ_DEVICE=1" in hdr
    core = open(os.path.join(ROOT, "include", "thermite.h")).read()
    assert "THM_N_TIMINGS = 8" in core and capi.N_TIMINGS == 8   # no timing slot of its own
    # the C compiler's layout of thm_fastq_upload_info against the ctypes structure
    fields = [f for f, _ in capi.FastqUploadInfo._fields_]
    assert fields == ["n_reads", "n_bases", "n_name_bytes", "on_device", "device_ms"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "thermite_io.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(thm_fastq_upload_info));\n' +
                   "".join('  printf(" %%zu", offsetof(thm_fastq_upload_info, %s));\n' % f for f in fields) +
                   '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True).stdout.split()]
    want = [ctypes.sizeof(capi.FastqUploadInfo)] + [getattr(capi.FastqUploadInfo, f).offset for f in fields]
    assert got == want and ctypes.sizeof(capi.FastqUploadInfo) == 32


def test_cpp_header_has_the_upload_call(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "thermite.hpp"\nauto p1 = &thermite::Aligner::upload_fastq;\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])


def test_null_arguments_need_no_device():
    L = capi.lib()
    info = capi.FastqUploadInfo()
    raw = ctypes.create_string_buffer(b"@r\nA\n+\nI\n")
    assert L.thm_batch_upload_fastq(None, raw, 9, b"p", 1, 1, ctypes.byref(info)) == capi.ERR_INVALID_ARG
    assert L.thm_batch_upload_fastq(None, None, 0, b"p", 1, 1, ctypes.byref(info)) == capi.ERR_INVALID_ARG
    assert L.thm_batch_upload_fastq(None, raw, 9, b"p", 1, 1, None) == capi.ERR_INVALID_ARG
    v = capi.ReadBatch()
    assert L.thm_batch_fetch_reads(None, ctypes.byref(v)) == capi.ERR_INVALID_ARG
    assert L.thm_batch_fetch_reads(None, None) == capi.ERR_INVALID_ARG
    n = ctypes.c_uint64(0)
    assert L.thm_debug_fastq_device_blocks(None, ctypes.byref(n), ctypes.byref(n)) == capi.ERR_INVALID_ARG


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fastq_model") / "fastq_model_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "thermite_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "fastq_model_main.cpp"), "-o", str(exe)])
    return exe


def _run_model(model, tmp_path, data):
    """-> None (declined) or the five arrays"""
    (tmp_path / "in.bin").write_bytes(data)
    subprocess.check_call([str(model), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = (tmp_path / "out.bin").read_bytes()
    if out == b"declined\n":
        return None
    assert out.startswith(b"parsed\n")
    at, got = 7, {}
    for k, dt in zip(fc.KEYS, (np.uint8, "<u8", np.uint8, "<u8", np.uint8)):
        n = int.from_bytes(out[at: at + 8], "little")
        got[k] = np.frombuffer(out[at + 8: at + 8 + n], dt)
        at += 8 + n
    assert at == len(out)
    return got


@pytest.mark.parametrize("name", list(_WELL))
def test_the_model_parses_every_well_formed_block_as_the_host_does(model, tmp_path, name):
    outcome, _ = fc.host_outcome(tmp_path, name, _WELL[name])
    assert outcome[0] == "batch"
    got = _run_model(model, tmp_path, _WELL[name])
    assert got is not None, "declined"
    assert fc.batches_differ(got, outcome[1]) is None, fc.batches_differ(got, outcome[1])
    if name == "long_read":
        assert int(np.diff(got["offsets"].astype(np.int64))[fc.LONG_READ_INDEX]) == fc.LONG_READ


@pytest.mark.parametrize("name", list(_DECLINED))
def test_the_model_declines_what_is_not_in_the_strict_form(model, tmp_path, name):
    block, last, ref = _DECLINED[name]
    assert _run_model(model, tmp_path, block) is None
    # what the host parser makes of it is an error, or a batch the device would not have produced from these bytes
    outcome, _ = fc.host_outcome(tmp_path, name, ref)
    assert outcome[0] in ("batch", "error")
    if outcome[0] == "error":
        assert outcome[1] == capi.ERR_FORMAT and ":" in outcome[2]
