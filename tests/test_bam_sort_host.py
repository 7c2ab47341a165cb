"""CPU side of the coordinate sort (include/thermite_io.h: thm_bam_sorter and the calls around it): the ABI, the sorted
header against the oracle's, and the order and the window addressing (thermite_amd/csrc/bam_sort_device.h, the functions
kernels_bam_sort.hip spreads over threads) run serially by tests/cpp/bam_sort_model_main.cpp against the expectation
of tests/bam_sort_common.py."""
import ctypes
import gzip
import os
import re
import subprocess

import pytest

import bam_common as bc
import bam_sort_common as sc
from oracle import aln_writer as ow
from thermite_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["thm_bam_sorter_create", "thm_bam_sorter_add", "thm_bam_sorter_finish", "thm_bam_sorter_next", "thm_bam_sorter_free",
               "thm_writer_header_sorted"]
HOOK = "thm_debug_bam_sorter_add_records"


# ------------------------------------------------------------------ ABI
def test_abi_symbols_and_struct_layouts(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "thermite_io.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in capi.IO_ABI_SYMBOLS
        assert hasattr(capi.lib(), s), "missing export: " + s
    assert hasattr(capi.lib(), HOOK) and HOOK not in hdr
    core = open(os.path.join(ROOT, "include", "thermite.h")).read()
    assert "THM_N_TIMINGS = 8" in core and len(capi.TIMING_NAMES) == capi.N_TIMINGS == 8
    structs = [("thm_bam_sort_info", capi.BamSortInfo), ("thm_bam_sorted_view", capi.BamSortedView)]
    src = tmp_path / "layout.c"
    body = ""
    for name, cls in structs:
        body += '  printf(" %%zu", sizeof(%s));\n' % name
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f, _ in cls._fields_)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "thermite_io.h"\nint main(void) {\n' + body +
                   '  printf(" %u %d\\n", THM_SORT_RAW, (int)THM_N_TIMINGS);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True).stdout.split()]
    want = []
    for name, cls in structs:
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    assert got == want + [capi.SORT_RAW, 8]
    assert [f for f, _ in capi.BamSortInfo._fields_] == ["n_reads", "n_records", "n_bytes", "total_records", "total_bytes", "n_failed_reads",
                                                        "read_status", "add_ms"]
    assert [f for f, _ in capi.BamSortedView._fields_] == ["total_records", "total_raw_bytes", "raw_offset", "n_raw_bytes", "n_blocks", "n_bytes",
                                                          "data", "block_off", "gather_ms", "deflate_ms"]
    assert ctypes.sizeof(capi.BamSortInfo) == 64 and ctypes.sizeof(capi.BamSortedView) == 72
    assert "THM_BAM_SORT=1" in hdr


def test_null_arguments_need_no_device():
    L = capi.lib()
    h = ctypes.c_void_p()
    info, view, text, ms = capi.BamSortInfo(), capi.BamSortedView(), capi.Text(), ctypes.c_float(0)
    assert L.thm_bam_sorter_create(None, 0, ctypes.byref(h)) == capi.ERR_INVALID_ARG and not h.value
    assert L.thm_bam_sorter_create(None, 0, None) == capi.ERR_INVALID_ARG
    assert L.thm_bam_sorter_add(None, 0, ctypes.byref(info)) == capi.ERR_INVALID_ARG
    assert L.thm_bam_sorter_finish(None, ctypes.byref(ms)) == capi.ERR_INVALID_ARG
    assert L.thm_bam_sorter_next(None, 0, 0, ctypes.byref(view)) == capi.ERR_INVALID_ARG
    assert L.thm_debug_bam_sorter_add_records(None, None, 0) == capi.ERR_INVALID_ARG
    assert L.thm_writer_header_sorted(None, ctypes.byref(text)) == capi.ERR_INVALID_ARG
    L.thm_bam_sorter_free(None)


# ------------------------------------------------------------------ header
@pytest.mark.parametrize("key", ["test_ref", "syn"])
def test_sorted_header_is_the_oracles_with_the_hd_line(key):
    t = bc.tables(key)
    ix = capi.Index(t)
    w = capi.Writer(ix, capi.FMT_BAM)
    assert gzip.decompress(w.header()) == ow.bam_header_bytes(t), "thm_writer_header changed"
    assert gzip.decompress(w.header_sorted()) == sc.sorted_header_bytes(t)
    assert gzip.decompress(w.header_sorted() + w.trailer()) == sc.sorted_header_bytes(t)   # a valid empty sorted BAM
    w.close()
    s = capi.Writer(ix, capi.FMT_SAM)
    assert s.header_sorted() == sc.HD_LINE + s.header() and s.header().startswith(b"@SQ")
    s.close()
    p = capi.Writer(ix, capi.FMT_PAF)
    assert p.header_sorted() == b"" == p.header()
    p.close()
    ix.close()
    if key == "test_ref":
        assert sc.n_sq_of(t) == 4


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bam_sort_model") / "bam_sort_model_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "thermite_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "bam_sort_model_main.cpp"), "-o", str(exe)])
    return exe


def _cases():
    cases = dict(sc.synthetic_cases(4))
    cases["golden"] = open(bc.GOLDEN_BIN, "rb").read()
    return cases


def test_golden_records_have_what_the_sort_is_checked_on():
    """four contigs in the header; among the records at least two refIDs, both strands, unmapped records and a tie"""
    recs = [bc.parse_record(r) for r in bc.split_records(open(bc.GOLDEN_BIN, "rb").read())]
    assert len({r["ref_id"] for r in recs if r["ref_id"] >= 0}) >= 2
    assert {r["flag"] & 16 for r in recs if r["ref_id"] >= 0} == {0, 16}
    assert sum(r["ref_id"] < 0 for r in recs) >= 2
    keys = sc.keys_of(bc.split_records(open(bc.GOLDEN_BIN, "rb").read()), 4)
    assert len(set(keys.tolist())) < len(keys), "no two records tie"
    assert max(keys.tolist()) >> 33 == 4, "the unmapped rank is n_sq, which log2(n_sq) bits would lose"


@pytest.mark.parametrize("window", [sc.BLOCK_IN, 3 * sc.BLOCK_IN], ids=["w1", "w3"])
@pytest.mark.parametrize("name", ["golden", "empty", "ties", "positions", "long_record"])
def test_model_gives_the_stably_sorted_stream(model, tmp_path, name, window):
    data = _cases()[name]
    want = sc.sorted_stream(data, 4)
    assert len(want) == len(data)
    (tmp_path / "in.bin").write_bytes(data)
    out = subprocess.run([str(model), str(tmp_path / "in.bin"), "4", str(window), str(tmp_path / "out.bin")], check=True,
                         capture_output=True, text=True).stdout.split()
    got = (tmp_path / "out.bin").read_bytes()
    assert got == want, name
    assert out == ["records", str(len(bc.split_records(data))), "bytes", str(len(data)), "windows", str(-(-len(data) // window))]
    if name == "long_record" and window == sc.BLOCK_IN:
        # one long record covers the whole first window, the other begins and ends inside windows
        recs = bc.split_records(want)
        assert bc.parse_record(recs[0])["qname"] == b"long_first" and len(recs[0]) > window
        k = [bc.parse_record(r)["qname"] for r in recs].index(b"long")
        at = sum(len(r) for r in recs[:k])
        assert at % window and (at + len(recs[k])) % window and at // window < (at + len(recs[k])) // window
    if name == "ties":
        names = [bc.parse_record(r)["qname"] for r in bc.split_records(want)]
        tied = [n for n in names if n.startswith(b"t")]
        assert len(tied) > 2990 and tied == sorted(tied, key=lambda n: int(n[1:]))
        assert names[0] == b"early" and names[-1] == b"unmapped" and names[-2] == b"reverse"
