"""CPU side of the coverage tracks (include/thermite_io.h: thm_coverage): the ABI, the expectation of tests/cov_common.py
on the golden SAM file against tables derived by hand, the functions the kernels spread over threads
(thermite_amd/csrc/coverage_device.h) run serially by tests/cpp/coverage_model_main.cpp against that expectation, and the
conditions the synthetic run must hold."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cigar_common as cc
import cov_common as cv
import quant_common as qc
from oracle import pyoracle as orc
from thermite_amd import capi, refdata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
SYMBOLS = ["thm_coverage_create", "thm_coverage_free", "thm_coverage_add", "thm_coverage_add_view", "thm_coverage_fetch", "thm_coverage_depth",
           "thm_coverage_reset"]
_memo = {}


def _syn():
    """(tables, oracle result) of the synthetic run, once"""
    if "syn" not in _memo:
        t = qc.syn_tables()
        bases, off = qc.syn_reads(t)
        r = orc.Index(t).align_batch(bases, off, capi.CI_OPTS, n_threads=8)
        assert r.counters[15] == 0
        _memo["syn"] = (t, r)
    return _memo["syn"]


def _shape_t():
    if "shape_t" not in _memo:
        _memo["shape_t"] = cv.shape_tables()
    return _memo["shape_t"]


# ------------------------------------------------------------------ ABI
def test_abi_symbols_and_layouts(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "thermite_io.h")).read()
    for s in SYMBOLS + ["thm_align_files"]:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in capi.IO_ABI_SYMBOLS and hasattr(capi.lib(), s), s
    structs = [("thm_cov_track_totals", capi.CovTrackTotals), ("thm_cov_totals", capi.CovTotals), ("thm_cov_info", capi.CovInfo),
               ("thm_cov_view", capi.CovView), ("thm_cov_depth_view", capi.CovDepthView)]
    body = ""
    for name, cls in structs:
        body += '  printf(" %%zu", sizeof(%s));\n' % name
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f, _ in cls._fields_)
    body += '  printf(" %zu", sizeof(thm_cov_run));\n'
    body += "".join('  printf(" %%zu", offsetof(thm_cov_run, %s));\n' % f for f in cv.RUN_DT.names)
    body += '  printf(" %u %u", THM_COV_STRANDED, THM_COV_MULTI);\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "thermite_io.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True).stdout.split()]
    want = []
    for _, cls in structs:
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    want += [24] + [cv.RUN_DT.fields[f][1] for f in cv.RUN_DT.names] + [cv.STRANDED, cv.MULTI]
    assert got == want
    assert ctypes.sizeof(capi.CovTotals) == 136 and [f for f, _ in capi.CovTotals._fields_][:5] == cv.TOTAL_NAMES
    assert capi.COV_RUN_DT == cv.RUN_DT and (capi.COV_STRANDED, capi.COV_MULTI) == (cv.STRANDED, cv.MULTI)
    assert "THM_COVERAGE=1" in hdr
    # the tile size capi mirrors is the header's, and it is what the shapes rely on
    dev = open(os.path.join(ROOT, "thermite_amd", "csrc", "coverage_device.h")).read()
    m = re.search(r"TILE_THREADS = (\d+), PER_THREAD = (\d+), TILE = TILE_THREADS \* PER_THREAD;", dev)
    assert m and int(m.group(1)) * int(m.group(2)) == capi.COV_TILE <= 65536
    assert re.search(r"static_assert\(TILE <= 65536", dev)


def test_null_arguments_need_no_device():
    L = capi.lib()
    h, info, view, dv, cview = ctypes.c_void_p(), capi.CovInfo(), capi.CovView(), capi.CovDepthView(), capi.CigarView()
    assert L.thm_coverage_create(None, 0, 0, ctypes.byref(h)) == capi.ERR_INVALID_ARG and not h
    assert L.thm_coverage_create(None, 0, 0, None) == capi.ERR_INVALID_ARG
    assert L.thm_coverage_add(None, ctypes.byref(info)) == capi.ERR_INVALID_ARG
    assert L.thm_coverage_add_view(None, ctypes.byref(cview), ctypes.byref(info)) == capi.ERR_INVALID_ARG
    assert L.thm_coverage_fetch(None, 0, 0, 0, ctypes.byref(view)) == capi.ERR_INVALID_ARG
    assert L.thm_coverage_depth(None, 0, 0, 0, 0, ctypes.byref(dv)) == capi.ERR_INVALID_ARG
    assert L.thm_coverage_reset(None) == capi.ERR_INVALID_ARG
    L.thm_coverage_free(None)


# ------------------------------------------------------------------ the golden file, counted by hand
@pytest.mark.parametrize("flags", cv.ALL_FLAGS)
def test_expectation_on_the_golden_sam_gives_the_hand_tables(flags):
    t = refdata.load_reference(DATA + "/test_ref.fasta", DATA + "/test_ref.gtf")
    sam = os.path.join(ROOT, "tests", "golden", "test_query.sam")
    e = cv.Expect(t, flags)
    e.add(*cv.sam_view(sam, t))
    cv.assert_golden(t, flags, e.runs, e.totals)
    cv.check_invariants(e)
    # ... and the line-by-line count of the same file agrees
    depth = cv.sam_depth(sam, t, flags)
    for k in range(cv.n_tracks(flags)):
        for s in range(4):
            assert np.array_equal(depth[k][s], e.depth(k, s)), (k, s)
        assert cv.bedgraph(qc.sq_names(t), depth[k]) == cv.bedgraph(qc.sq_names(t), [e.depth(k, s) for s in range(4)])
    if flags == 0:
        assert cv.bedgraph(qc.sq_names(t), depth[0]).startswith("another_seq\t8\t12\t1\nintrons_seq\t5\t7\t3\n")


@pytest.mark.parametrize("flags", cv.ALL_FLAGS)
def test_expectation_on_the_oracle_of_the_golden_reads(flags):
    t = refdata.load_reference(DATA + "/test_ref.fasta", DATA + "/test_ref.gtf")
    _, seqs, _ = refdata.parse_fastq(DATA + "/test_query.fastq")
    bases, off = refdata.pack_reads(seqs)
    r = orc.Index(t).align_batch(bases, off, dict(capi.DEFAULT_OPTS, min_seed_len=3, min_aln_score=0))
    e = cv.from_oracle(t, flags, r)
    cv.assert_golden(t, flags, e.runs, e.totals)


def test_blocks_of_the_contracts_examples():
    w = lambda cigar: [(n << 4) | cc.BAM_CODE[c] for n, c in cigar]
    assert cv.blocks_of(w([(3, "M"), (2, "D"), (4, "M")]), 10) == [(10, 19)]
    assert cv.blocks_of(w([(3, "M"), (4, "N"), (4, "M")]), 10) == [(10, 13), (17, 21)]
    assert cv.blocks_of(w([(2, "S"), (3, "M"), (5, "I"), (1, "M"), (7, "N"), (6, "N"), (2, "M"), (1, "S")]), 0) == [(0, 4), (17, 19)]
    assert cv.track_names(3) == ["unique.fwd", "unique.rev", "multi.fwd", "multi.rev"] and cv.track_names(0) == ["unique"]
    assert [cv.track_of(3, m, f) for m in (0, 1) for f in (1, 0)] == [0, 1, 2, 3] and cv.track_of(1, True, True) is None


# ------------------------------------------------------------------ the synthetic run holds what it is meant to test
def test_coverage_conditions_of_the_synthetic_run():
    t, r = _syn()
    e = cv.from_oracle(t, cv.STRANDED | cv.MULTI, r)
    cv.check_invariants(e)
    tot = e.totals
    assert tot["n_alns"] == len(r.alns) and tot["n_skipped_multi"] == 0
    # reads on both strands, unique and multi-mapped; spliced alignments; depths of 2 and more
    assert all(tot["track"][k]["n_alns"] >= 20 for k in range(4)), tot
    assert any(tot["track"][k]["n_blocks"] > tot["track"][k]["n_alns"] for k in range(4))
    assert max(int(e.runs(k)["depth"].max()) for k in range(4)) >= 2
    assert sum(len(e.runs(k)) for k in range(4)) >= 1000
    plain = cv.from_oracle(t, 0, r)
    assert plain.totals["n_skipped_multi"] >= 40


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = tmp_path_factory.mktemp("coverage_model") / "coverage_model_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "thermite_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "coverage_model_main.cpp"), "-o", str(exe)])
    return exe


def _run_model(model, tmp_path, data):
    (tmp_path / "in.bin").write_bytes(data)
    p = subprocess.run([str(model), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True)
    return p.returncode, (tmp_path / "out.bin").read_bytes() if p.returncode == 0 else p.stderr


def _check_model(model, tmp_path, t, flags, views, windows, what):
    rc, out = _run_model(model, tmp_path, cv.model_input(t, flags, views, windows))
    assert rc == 0, out
    e = cv.Expect(t, flags)
    for v in views:
        e.add(*v)
    tot, runs, depths = cv.model_output(flags, windows, out)
    assert tot == e.totals, (what, tot, e.totals)
    for k in range(cv.n_tracks(flags)):
        cv.assert_runs_equal(runs[k], e.runs(k), "%s track %d" % (what, k))
    for (k, s, start, n), d in zip(windows, depths):
        assert np.array_equal(d, e.depth(k, s)[start: start + n]), (what, k, s, start, n)
    cv.check_invariants(e)
    return e


SHAPES = ["empty", "no_alignments", "whole_contig", "abutting", "tile_span", "tile_edge", "hot", "forty_introns", "one_read_5000", "both_strands", "long_run",
          "later_add"]


@pytest.mark.parametrize("name", SHAPES)
def test_model_gives_the_expected_tracks_on_the_shapes(model, tmp_path, name):
    t = _shape_t()
    views = cv.shape_cases(t, capi.COV_TILE)[name]
    for flags in (0, cv.STRANDED | cv.MULTI):
        windows = [w for w in cv.shape_windows(capi.COV_TILE) if w[0] < cv.n_tracks(flags)]
        e = _check_model(model, tmp_path, t, flags, views, windows, "%s flags %d" % (name, flags))
        cv.assert_shape(name, flags, e, capi.COV_TILE)


def test_model_on_the_oracle_of_the_synthetic_run(model, tmp_path):
    t, r = _syn()
    dig, words = cc.expected_alignments(r.alns, r.ops)
    n = cv.sq_lengths(t)[0]
    for flags in cv.ALL_FLAGS:
        windows = [(0, 0, 0, 1), (0, 0, n - 1, 1), (cv.n_tracks(flags) - 1, 0, capi.COV_TILE + 17, 3 * capi.COV_TILE), (0, 0, n - 5000, 5000)]
        _check_model(model, tmp_path, t, flags, [(r.offsets, r.alns, dig, words)], windows, "synthetic run flags %d" % flags)


@pytest.mark.parametrize("name", ["past_the_contig", "no_refid", "outside_the_pool"])
def test_model_refuses_and_adds_nothing(model, tmp_path, name):
    t = _shape_t()
    bad = cv.bad_views(t)[name]
    good = cv.shape_cases(t, capi.COV_TILE)["abutting"][0]
    assert _run_model(model, tmp_path, cv.model_input(t, 3, [good]))[0] == 0
    assert _run_model(model, tmp_path, cv.model_input(t, 3, [bad]))[0] == 3
    assert _run_model(model, tmp_path, cv.model_input(t, 3, [good, bad]))[0] == 3
    if name == "past_the_contig":
        # one base less and it fits: the run ends exactly at the contig's length
        off, alns, dig, words = bad
        words = words.copy()
        words[-1] -= 1 << 4
        rc, out = _run_model(model, tmp_path, cv.model_input(t, 0, [(off, alns, dig, words)]))
        assert rc == 0
        assert cv.table(cv.model_output(0, (), out)[1][0], 1) == [(950, 970, 1), (980, 1000, 1)]
