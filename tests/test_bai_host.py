"""CPU side of the BAI index (include/thermite_io.h: thm_bam_sorter_index): the ABI, the functions the kernels spread
over threads (thermite_amd/csrc/bai_device.h) run serially by tests/cpp/bai_model_main.cpp against the expectation of
tests/bai_common.py, and that expectation against itself: a region query written from the SAM specification must find,
through the expected index, every mapped record a walk of the whole stream finds."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import bai_common as xc
import bam_sort_common as sc
from thermite_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SQ = 4
HEADER = xc.bgzf_member(bytes(np.random.default_rng(5).integers(0, 256, 6000, dtype=np.uint8)))   # stands where a BAM header would
FIRST = len(HEADER)   # where the first record member stands in the made-up files
_cache = {}


def _case(name):
    """(sorted stream, members, file) of a synthetic case"""
    if name not in _cache:
        stream = sc.sorted_stream(xc.synthetic_cases(N_SQ)[name], N_SQ)
        members = xc.bgzf_members(stream)
        _cache[name] = (stream, members, HEADER + b"".join(members) + xc.EOF_BLOCK)
    return _cache[name]


CASES = ["empty", "one_reference", "bin_levels", "no_span", "linear", "merge", "member_cuts", "many"]


# ------------------------------------------------------------------ ABI
def test_abi_symbol_and_view_layout(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "thermite_io.h")).read()
    assert re.search(r"\bthm_bam_sorter_index\s*\(", hdr)
    assert "thm_bam_sorter_index" in capi.IO_ABI_SYMBOLS and hasattr(capi.lib(), "thm_bam_sorter_index")
    src = tmp_path / "layout.c"
    body = '  printf(" %zu", sizeof(thm_bai_view));\n' + "".join('  printf(" %%zu", offsetof(thm_bai_view, %s));\n' % f for f, _ in capi.BaiView._fields_)
    body += '  printf(" %zu %zu", sizeof(thm_bam_sorted_view), sizeof(thm_bam_sort_info));\n'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "thermite_io.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True).stdout.split()]
    want = [ctypes.sizeof(capi.BaiView)] + [getattr(capi.BaiView, f).offset for f, _ in capi.BaiView._fields_] + [72, 64]
    assert got == want
    assert [f for f, _ in capi.BaiView._fields_] == ["n_bytes", "data", "n_refs", "n_bins", "n_chunks", "n_intervals", "n_no_coor", "index_ms"]
    assert "THM_BAM_INDEX=1" in hdr and "an index file" not in hdr


def test_null_arguments_need_no_device():
    L = capi.lib()
    v = capi.BaiView()
    assert L.thm_bam_sorter_index(None, 0, ctypes.byref(v)) == capi.ERR_INVALID_ARG
    assert L.thm_bam_sorter_index(None, 0, None) == capi.ERR_INVALID_ARG


def test_one_reg2bin_in_the_sources():
    """the writer, the record encoder and the index call the function of bai_device.h"""
    csrc = os.path.join(ROOT, "thermite_amd", "csrc")
    defs = [f for f in sorted(os.listdir(csrc)) if re.search(r"uint32_t reg2bin\(", open(os.path.join(csrc, f)).read())]
    assert defs == ["bai_device.h"]


# ------------------------------------------------------------------ the cases are what they are meant to be
def test_the_cases_hold_what_they_test():
    ix = {name: xc.expected_index(_case(name)[0], N_SQ, [len(m) for m in _case(name)[1]], FIRST) for name in CASES}
    r = ix["one_reference"]["refs"]
    assert [x["pseudo"] is None for x in r] == [True, True, False, True] and ix["one_reference"]["n_no_coor"] == 20
    assert r[0]["bins"] == [] and r[0]["ioffset"] == [] and r[2]["pseudo"][1] == (300, 0)
    # a record that ends on a boundary stays in the 16 kb bin; one base more and it is in the bin of the level above
    bins = {b for b, _ in ix["bin_levels"]["refs"][0]["bins"]}
    for k, b in enumerate(xc.BOUNDARIES):
        assert xc.reg2bin(b - 100, b) == 4681 + (b - 1 >> 14) and xc.reg2bin(b - 100, b) in bins
        up = xc.reg2bin(b - 100, b + 1)
        assert up in bins and up < 4681 and (k == 4 and up == 0 or up == (0, 1, 9, 73, 585)[4 - k] + (b >> (17 + 3 * k)))
    for x in ix["no_span"]["refs"]:
        assert all(4681 <= b for b, _ in x["bins"])
    lin = ix["linear"]["refs"][0]
    assert len(lin["ioffset"]) == 142 and lin["pseudo"][1] == (4, 2)            # un_top, alone in window 200, does not count
    assert lin["ioffset"][1] == lin["ioffset"][5] < lin["ioffset"][6] == lin["ioffset"][100] < lin["ioffset"][101] == lin["ioffset"][141]
    assert ix["linear"]["refs"][1]["ioffset"] == [] and ix["linear"]["refs"][1]["pseudo"][1] == (0, 1)
    parent = xc.reg2bin(5 * xc.W - 30, 5 * xc.W + 20)
    m = ix["merge"]["refs"]
    assert len(dict(m[0]["bins"])[parent]) == 1 and len(dict(m[1]["bins"])[parent]) == 4
    stream = _case("member_cuts")[0]
    recs = xc.split_records(stream)
    assert len(recs[0]) == xc.CUT and len(stream) % xc.CUT == 0
    cuts = ix["member_cuts"]["refs"]
    assert cuts[0]["bins"][0][1][0][0] & 0xffff == 0 or cuts[0]["bins"][0][1][0][1] & 0xffff == 0
    assert cuts[3]["pseudo"][0][1] == (FIRST + sum(len(x) for x in _case("member_cuts")[1])) << 16   # the trailer member, offset 0
    assert sum(len(x["bins"]) for x in ix["many"]["refs"]) > 300 and ix["many"]["n_no_coor"] > 1000


# ------------------------------------------------------------------ the contract against itself
@pytest.mark.parametrize("name", CASES)
def test_a_query_through_the_expected_index_finds_every_mapped_record(name):
    stream, members, bam = _case(name)
    data = xc.expected_bai(stream, N_SQ, [len(m) for m in members], FIRST)
    index = xc.parse_bai(data)
    assert index == xc.expected_index(stream, N_SQ, [len(m) for m in members], FIRST) and xc.index_bytes(index) == data
    regions = xc.regions_of(stream, N_SQ)
    if name == "many":   # (every region walks thousands of records here)
        regions = regions[::3]
    assert any(xc.brute_force(stream, *r) for r in regions) or name == "empty"
    xc.check_queries(index, bam, stream, N_SQ, regions)


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bai_model") / "bai_model_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "thermite_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "bai_model_main.cpp"), "-o", str(exe)])
    return exe


@pytest.mark.parametrize("first", [0, FIRST, 2 ** 32 + 12345], ids=["f0", "fhdr", "f2p32"])
@pytest.mark.parametrize("name", CASES)
def test_model_gives_the_expected_index(model, tmp_path, name, first):
    stream, members, _ = _case(name)
    sizes = np.array([len(m) for m in members], "<u8")
    (tmp_path / "in.bin").write_bytes(stream)
    (tmp_path / "sizes.bin").write_bytes(sizes.tobytes())
    subprocess.run([str(model), str(tmp_path / "in.bin"), str(N_SQ), str(tmp_path / "sizes.bin"), str(first), str(tmp_path / "out.bai")], check=True)
    assert (tmp_path / "out.bai").read_bytes() == xc.expected_bai(stream, N_SQ, sizes, first)


def test_model_refuses_a_record_beyond_2_pow_29(model, tmp_path):
    stream = xc.make_record(1, 2 ** 31 - 2, 0, b"far", 4, [("M", 4)])
    (tmp_path / "in.bin").write_bytes(stream)
    (tmp_path / "sizes.bin").write_bytes(np.array([60], "<u8").tobytes())
    rc = subprocess.run([str(model), str(tmp_path / "in.bin"), str(N_SQ), str(tmp_path / "sizes.bin"), "0", str(tmp_path / "out.bai")]).returncode
    assert rc == 3
    edge = xc.make_record(1, 2 ** 29 - 4, 0, b"edge", 4, [("M", 4)])   # ends on 2^29: the last addressable base
    (tmp_path / "in.bin").write_bytes(edge)
    subprocess.run([str(model), str(tmp_path / "in.bin"), str(N_SQ), str(tmp_path / "sizes.bin"), "0", str(tmp_path / "out.bai")], check=True)
    assert (tmp_path / "out.bai").read_bytes() == xc.expected_bai(edge, N_SQ, [60], 0)
