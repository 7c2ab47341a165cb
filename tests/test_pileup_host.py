"""CPU side of the per-base allele counts (include/thermite_io.h: thm_pileup): the ABI, the expectation of
tests/pileup_common.py against the line-by-line count of a SAM file and the FASTA, the functions the kernels spread over
lanes (thermite_amd/csrc/pileup_device.h) run serially by tests/cpp/pileup_model_main.cpp against that expectation, and
the conditions the synthetic run and the shapes must hold."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cigar_common as cc
import pileup_common as pc
import quant_common as qc
from oracle import aln_writer as ow
from oracle import pyoracle as orc
from thermite_amd import capi, refdata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
SYMBOLS = ["thm_pileup_create", "thm_pileup_free", "thm_pileup_add", "thm_pileup_add_view", "thm_pileup_fetch", "thm_pileup_window", "thm_pileup_reset"]
CHUNK, GROUP, TILE = capi.PILE_CHUNK, capi.PILE_GROUP, capi.COV_TILE
_memo = {}


def _syn():
    """(tables, reads, offsets, oracle result) of the synthetic run, once"""
    if "syn" not in _memo:
        t = qc.syn_tables()
        bases, off = qc.syn_reads(t)
        r = orc.Index(t).align_batch(bases, off, capi.CI_OPTS, n_threads=8)
        assert r.counters[15] == 0
        _memo["syn"] = (t, bases, off, r)
    return _memo["syn"]


def _shape_t():
    if "shape_t" not in _memo:
        _memo["shape_t"] = pc.shape_tables()
    return _memo["shape_t"]


def _shapes():
    if "shapes" not in _memo:
        _memo["shapes"] = pc.shape_cases(_shape_t(), CHUNK, GROUP, TILE)
    return _memo["shapes"]


# ------------------------------------------------------------------ ABI
def test_abi_symbols_and_layouts(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "thermite_io.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in capi.IO_ABI_SYMBOLS and hasattr(capi.lib(), s), s
    structs = [("thm_pile_totals", capi.PileTotals), ("thm_pile_info", capi.PileInfo), ("thm_pile_view", capi.PileView)]
    body = ""
    for name, cls in structs:
        body += '  printf(" %%zu", sizeof(%s));\n' % name
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f, _ in cls._fields_)
    body += '  printf(" %zu", sizeof(thm_pile_site));\n'
    body += "".join('  printf(" %%zu", offsetof(thm_pile_site, %s));\n' % f for f in pc.SITE_DT.names)
    body += '  printf(" %u", THM_PILE_MULTI);\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "thermite_io.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True).stdout.split()]
    want = []
    for _, cls in structs:
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    want += [48] + [pc.SITE_DT.fields[f][1] for f in pc.SITE_DT.names] + [pc.MULTI]
    assert got == want
    assert ctypes.sizeof(capi.PileTotals) == 96 and [f for f, _ in capi.PileTotals._fields_] == pc.TOTAL_NAMES
    assert capi.PILE_SITE_DT == pc.SITE_DT and capi.PILE_MULTI == pc.MULTI
    assert "THM_PILEUP=1" in hdr and "THM_PILEUP_MIN_ALT" in hdr
    # the chunk and group sizes capi mirrors are the header's: the shapes place their edges by them
    dev = open(os.path.join(ROOT, "thermite_amd", "csrc", "pileup_device.h")).read()
    m = re.search(r"constexpr uint32_t CHUNK = (\d+), GROUP = (\d+);", dev)
    assert m and (int(m.group(1)), int(m.group(2))) == (CHUNK, GROUP)
    assert re.search(r"MAX_WINDOW = 1ull << 20;", dev) and capi.PILE_MAX_WINDOW == 1 << 20


def test_null_arguments_need_no_device():
    L = capi.lib()
    h, info, view, cview = ctypes.c_void_p(), capi.PileInfo(), capi.PileView(), capi.CigarView()
    assert L.thm_pileup_create(None, 0, 0, ctypes.byref(h)) == capi.ERR_INVALID_ARG and not h
    assert L.thm_pileup_create(None, 0, 0, None) == capi.ERR_INVALID_ARG
    assert L.thm_pileup_add(None, ctypes.byref(info)) == capi.ERR_INVALID_ARG
    assert L.thm_pileup_add_view(None, ctypes.byref(cview), None, None, ctypes.byref(info)) == capi.ERR_INVALID_ARG
    assert L.thm_pileup_fetch(None, 0, 0, 1, ctypes.byref(view)) == capi.ERR_INVALID_ARG
    assert L.thm_pileup_window(None, 0, 0, 0, ctypes.byref(view)) == capi.ERR_INVALID_ARG
    assert L.thm_pileup_reset(None) == capi.ERR_INVALID_ARG
    L.thm_pileup_free(None)


# ------------------------------------------------------------------ the golden file: the expectation and the second count
@pytest.mark.parametrize("flags", [0, pc.MULTI])
def test_expectation_on_the_golden_sam_gives_the_hand_rows(flags):
    t = refdata.load_reference(DATA + "/test_ref.fasta", DATA + "/test_ref.gtf")
    sam = os.path.join(ROOT, "tests", "golden", "test_query.sam")
    names = qc.sq_names(t)
    e = pc.Expect(t, flags)
    e.add(*pc.sam_view(sam, t))
    pc.check_invariants(e)
    rows = pc.sam_pileup(sam, pc.parse_fasta_text(DATA + "/test_ref.fasta"), names, multi=bool(flags), min_alt=1)
    assert pc.rows_as_tuples(names, e.rows()) == rows
    # spliced_with_err1 shows a C where three other reads show the T; spliced_revcomp_err1 an A where one other shows it
    assert rows == [("introns_seq", 21, "T", 4, 0, 1, 0, 3, 0, 0, 0), ("introns_revcomp", 20, "T", 2, 1, 0, 0, 1, 0, 0, 0)]
    assert (e.totals["n_reads"], e.totals["n_alns"], e.totals["n_used_alns"], e.totals["n_mismatches"]) == (10, 9, 9 if flags else 7, 2)


def test_expectation_against_the_second_count_on_the_oracles_sam(tmp_path):
    t, bases, off, r = _syn()
    names = qc.sq_names(t)
    sam = tmp_path / "syn.sam"
    n = len(off) - 1
    seqs = [bytes(bases[int(off[i]): int(off[i + 1])]) for i in range(n)]
    sam.write_bytes(ow.sam_header(t) + ow.format_batch(t, [b"r%d" % i for i in range(n)], seqs, [b"I" * len(x) for x in seqs], r, "sam"))
    fasta = [(names[s], bytes(seq).decode()) for s, seq in enumerate(pc.contig_seqs(t))]
    view = pc.sam_view(str(sam), t)
    for flags in (0, pc.MULTI):
        e = pc.from_oracle(t, flags, r, bases, off)
        pc.check_invariants(e)
        # the view read back from the SAM text gives the same counts as the oracle's arrays ...
        e2 = pc.Expect(t, flags)
        e2.add(*view)
        assert e2.totals == e.totals and all((a == b).all() for a, b in zip(e.cnt, e2.cnt))
        # ... and the line-by-line count agrees at both thresholds, as rows and as the driver's file
        for min_alt in (1, 2):
            rows = pc.sam_pileup(str(sam), fasta, names, multi=bool(flags), min_alt=min_alt)
            assert pc.rows_as_tuples(names, e.rows(min_alt=min_alt)) == rows
            assert pc.tsv(names, e.rows(min_alt=min_alt)) == pc.tsv_of_sam(rows)


def test_pileup_conditions_of_the_synthetic_run():
    t, bases, off, r = _syn()
    e, em = pc.from_oracle(t, 0, r, bases, off), pc.from_oracle(t, pc.MULTI, r, bases, off)
    tot = e.totals
    assert tot["n_alns"] == len(r.alns) and tot["n_skipped_multi"] >= 40 and em.totals["n_skipped_multi"] == 0
    assert tot["n_mismatches"] >= 1000 and tot["n_blocks"] > tot["n_used_alns"]
    assert len(e.rows(min_alt=1)) > len(e.rows(min_alt=2)) > 0
    # the reads are over ACGTN only, so a mismatch is what the oracle counts as a substitution
    assert set(np.unique(bases)) <= set(b"ACGTN")
    dig, _ = cc.expected_alignments(r.alns, r.ops)
    assert em.totals["n_mismatches"] == int(dig["n_subst"].sum())
    uniq = np.repeat(np.diff(r.offsets.astype(np.int64)) == 1, np.diff(r.offsets.astype(np.int64)))
    assert tot["n_mismatches"] == int(dig["n_subst"][uniq].sum())


def test_shapes_hold_what_they_are_there_for():
    t = _shape_t()
    exp = {}
    for name, views in _shapes().items():
        for flags in (0, pc.MULTI):
            e = pc.Expect(t, flags)
            for v in views:
                e.add(*v)
            pc.check_invariants(e)
            exp[(name, flags)] = e
    site = lambda e, s, x: e.window(s, x, 1)[0]
    assert len(exp[("perfect", 0)].rows()) == 0 and exp[("perfect", 0)].totals["n_m_bases"] == 182
    assert [(int(r["ref_id"]), int(r["pos"])) for r in exp[("contig_ends", 0)].rows()] == [(1, 0), (1, 999), (2, pc.CONTIG - 1)]
    for op in "SIDN":
        assert exp[("next_to_" + op, 0)].totals["n_mismatches"] == (2 if op == "S" else 4), op
    e = exp[("ins_behind_s_and_n", 0)]
    assert site(e, 0, 600)["ins"] == 1 and site(e, 0, 724)["ins"] == 1 and site(e, 0, 724)["depth"] == 0 and site(e, 0, 900)["ins"] == 2
    e = exp[("d_next_to_n", 0)]
    assert [int(site(e, 0, 1500 + k)["del"]) for k in (4, 5, 6, 7, 36, 37, 39, 40)] == [0, 1, 1, 0, 0, 1, 1, 0]
    e = exp[("reverse_ends", 0)]
    assert [int(r["pos"]) for r in e.rows(0, 1)] == [2500, 2590] and [int(r["pos"]) for r in e.rows(2, 1)] == [2500, 2539]
    e = exp[("lengths", 0)]
    assert e.totals["n_used_alns"] == 13 and e.totals["n_mismatches"] > 2 * 5000 // CHUNK
    assert exp[("forty_introns", 0)].totals["n_blocks"] == 2 * 41 and exp[("forty_introns", 0)].totals["n_ins"] == 2 * 20
    r = exp[("hot_same_mismatch", 0)].rows()
    assert len(r) == 1 and int(r[0]["depth"]) == 5000 and sorted(r[0]["cnt"].tolist()) == [0, 0, 0, 0, 5000] and r[0]["cnt"][pc.KIND[r[0]["ref_base"]]] == 0
    r = site(exp[("hot_every_kind", 0)], 0, 9000)
    assert all(x > 0 for x in r["cnt"]) and r["del"] == 1 and r["ins"] == 1 and r["depth"] == 16
    n_rows = [len(exp[("hot_every_kind", 0)].rows(min_alt=k)) for k in (1, 2, 3, 4)]       # rows on both sides of every filter
    assert n_rows == [4, 3, 2, 1], n_rows
    assert [(int(r["ref_id"]), int(r["pos"])) for r in exp[("tile_edges", 0)].rows()] == [(0, TILE - 1), (0, TILE), (0, 3 * TILE + 104), (2, 2 * TILE - 1), (2, 2 * TILE)]
    e = exp[("letters", 0)]
    assert [int(r["pos"]) for r in e.rows(0, 1)] == [301, 1102, 1105, 1107, 1108] and site(e, 0, 300)["cnt"][4] == 1 and site(e, 0, 7000)["cnt"][4] == 1
    assert exp[("long_run", 0)].totals["n_long_run_alns"] == 1 and exp[("long_run", 0)].totals["n_used_alns"] == 1
    assert exp[("multi", 0)].totals["n_skipped_multi"] == 2 and exp[("multi", pc.MULTI)].totals["n_used_alns"] == 3
    assert len(exp[("multi", pc.MULTI)].rows()) > len(exp[("multi", 0)].rows()) == 1


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pileup_model") / "pileup_model_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "thermite_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "pileup_model_main.cpp"), "-o", str(exe)])
    return exe


def _run_model(model, tmp_path, data):
    (tmp_path / "in.bin").write_bytes(data)
    p = subprocess.run([str(model), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True)
    return p.returncode, (tmp_path / "out.bin").read_bytes() if p.returncode == 0 else p.stderr


def _check_model(model, tmp_path, t, flags, views, windows, what):
    rc, out = _run_model(model, tmp_path, pc.model_input(t, flags, views, windows))
    assert rc == 0, out
    e = pc.Expect(t, flags)
    for v in views:
        e.add(*v)
    tot, n_events, fetches, wins = pc.model_output(windows, out)
    assert tot == e.totals, (what, tot, e.totals)
    assert n_events == e.n_events(), what
    for k, rows in enumerate(fetches):
        pc.assert_sites_equal(rows, e.rows(min_alt=k + 1), "%s min_alt %d" % (what, k + 1))
    for (s, start, n), rows in zip(windows, wins):
        pc.assert_sites_equal(rows, e.window(s, start, n), "%s window %d %d +%d" % (what, s, start, n))
    return e


SHAPES = ["empty", "no_alignments", "perfect", "contig_ends", "next_to_S", "next_to_I", "next_to_D", "next_to_N", "ins_behind_s_and_n", "d_next_to_n",
          "reverse_ends", "lengths", "forty_introns", "hot_same_mismatch", "hot_every_kind", "tile_edges", "letters", "long_run", "multi", "later_add"]


def test_the_shape_list_is_complete():
    assert sorted(SHAPES) == sorted(_shapes())


@pytest.mark.parametrize("name", SHAPES)
def test_model_gives_the_expected_counts_on_the_shapes(model, tmp_path, name):
    for flags in (0, pc.MULTI):
        _check_model(model, tmp_path, _shape_t(), flags, _shapes()[name], pc.shape_windows(TILE), "%s flags %d" % (name, flags))


def test_model_on_the_oracle_of_the_synthetic_run(model, tmp_path):
    t, bases, off, r = _syn()
    dig, words = cc.expected_alignments(r.alns, r.ops)
    n = len(pc.contig_seqs(t)[0])
    for flags in (0, pc.MULTI):
        windows = [(0, 0, 1), (0, n - 1, 1), (0, TILE + 17, 3 * TILE), (0, n - 5000, 5000)]
        _check_model(model, tmp_path, t, flags, [(r.offsets, r.alns, dig, words, bases, off)], windows, "synthetic run flags %d" % flags)


@pytest.mark.parametrize("name", ["past_the_contig", "query_length"])
def test_model_refuses_and_adds_nothing(model, tmp_path, name):
    t = _shape_t()
    bad = pc.bad_views(t)[name]
    good = _shapes()["perfect"][0]
    assert _run_model(model, tmp_path, pc.model_input(t, 1, [good]))[0] == 0
    assert _run_model(model, tmp_path, pc.model_input(t, 1, [bad]))[0] == 3
    assert _run_model(model, tmp_path, pc.model_input(t, 1, [good, bad]))[0] == 3
