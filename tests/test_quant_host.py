"""CPU side of the gene and junction count tables (include/thermite_io.h: thm_quant): the ABI, the expectation of
tests/quant_common.py on the golden SAM file against tables derived by hand, the functions the kernels spread over threads
(thermite_amd/csrc/quant_device.h) run serially by tests/cpp/quant_model_main.cpp against that expectation, and the
synthetic run's coverage conditions."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cigar_common as cc
import quant_common as qc
from oracle import pyoracle as orc
from thermite_amd import capi, refdata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
SYMBOLS = ["thm_quant_create", "thm_quant_free", "thm_quant_add", "thm_quant_add_view", "thm_quant_fetch", "thm_quant_reset"]
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


# ------------------------------------------------------------------ ABI
def test_abi_symbols_and_layouts(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "thermite_io.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in capi.IO_ABI_SYMBOLS and hasattr(capi.lib(), s), s
    structs = [("thm_quant_totals", capi.QuantTotals), ("thm_quant_info", capi.QuantInfo), ("thm_quant_view", capi.QuantView)]
    body = ""
    for name, cls in structs:
        body += '  printf(" %%zu", sizeof(%s));\n' % name
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f, _ in cls._fields_)
    body += '  printf(" %zu %zu", sizeof(thm_quant_gene), sizeof(thm_quant_junction));\n'
    body += "".join('  printf(" %%zu", offsetof(thm_quant_junction, %s));\n' % (f if f != "pad" else "pad_") for f in qc.JUNCTION_DT.names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "thermite_io.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True).stdout.split()]
    want = []
    for _, cls in structs:
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    want += [32, 48] + [qc.JUNCTION_DT.fields[f][1] for f in qc.JUNCTION_DT.names]
    assert got == want
    assert ctypes.sizeof(capi.QuantTotals) == 88 and [f for f, _ in capi.QuantTotals._fields_] == qc.TOTAL_NAMES
    assert capi.QUANT_GENE_DT == qc.GENE_DT and capi.QUANT_JUNCTION_DT == qc.JUNCTION_DT
    assert "THM_QUANT=1" in hdr


def test_null_arguments_need_no_device():
    L = capi.lib()
    h, info, view, cv = ctypes.c_void_p(), capi.QuantInfo(), capi.QuantView(), capi.CigarView()
    assert L.thm_quant_create(None, ctypes.byref(h)) == capi.ERR_INVALID_ARG and not h
    assert L.thm_quant_create(None, None) == capi.ERR_INVALID_ARG
    assert L.thm_quant_add(None, ctypes.byref(info)) == capi.ERR_INVALID_ARG
    assert L.thm_quant_add_view(None, ctypes.byref(cv), ctypes.byref(info)) == capi.ERR_INVALID_ARG
    assert L.thm_quant_fetch(None, ctypes.byref(view)) == capi.ERR_INVALID_ARG
    assert L.thm_quant_reset(None) == capi.ERR_INVALID_ARG
    L.thm_quant_free(None)


# ------------------------------------------------------------------ the golden file, counted by hand
def test_expectation_on_the_golden_sam_gives_the_hand_tables():
    t = refdata.load_reference(DATA + "/test_ref.fasta", DATA + "/test_ref.gtf")
    sam = os.path.join(ROOT, "tests", "golden", "test_query.sam")
    qc.assert_golden(t, qc.expected_tables(t, *qc.sam_view(sam, t)))
    # ... and the line-by-line count of the same file agrees (spliced_with_err2's 3S1M12N4M is the (8, 20) hit with overhang 1)
    genes, rows = qc.count_sam(sam, t)
    assert {g: tuple(v) for g, v in genes.items()} == qc.GOLDEN_GENES
    assert sorted((qc.sq_names(t).index(k[0]), k[1], k[2], k[3], v[0], v[2]) for k, v in rows.items()) == qc.GOLDEN_JUNCTIONS
    assert any(c == "3S1M12N4M" for _, _, _, _, c, _ in qc._sam_records(sam))
    x = qc.expected_tables(t, *qc.sam_view(sam, t))
    assert qc.tsv_of(t, x) == qc.tsv_of_sam_counts(t, genes, rows)


def test_expectation_on_the_oracle_of_the_golden_reads():
    t = refdata.load_reference(DATA + "/test_ref.fasta", DATA + "/test_ref.gtf")
    _, seqs, _ = refdata.parse_fastq(DATA + "/test_query.fastq")
    bases, off = refdata.pack_reads(seqs)
    r = orc.Index(t).align_batch(bases, off, dict(capi.DEFAULT_OPTS, min_seed_len=3, min_aln_score=0))
    qc.assert_golden(t, qc.from_oracle(t, r))


# ------------------------------------------------------------------ the synthetic run holds what it is meant to test
def test_coverage_conditions_of_the_synthetic_run():
    t, r = _syn()
    x = qc.from_oracle(t, r)
    qc.check_invariants(x)
    tot = x["totals"]
    assert len(x["junctions"]) >= 200
    # junctions reached through two or more transcripts
    dig, words = cc.expected_alignments(r.alns, r.ops)
    via = {}
    for a in range(len(r.alns)):
        if int(r.alns[a]["aln_type"]) != qc.EXONIC:
            continue
        o = int(dig[a]["cigar_off"])
        for s, e, _ in qc.junction_hits(words[o: o + int(dig[a]["n_cigar"])], r.alns[a]["ystart"]):
            via.setdefault((s, e), set()).add(int(r.alns[a]["tx_or_gene_idx"]))
    assert sum(1 for v in via.values() if len(v) >= 2) >= 10
    assert tot["n_multi_reads"] >= 20
    assert int(x["genes"]["intronic_unique"].sum() + x["genes"]["intronic_multi"].sum()) >= 5
    assert tot["n_unmapped_reads"] >= 1
    assert tot["n_spliced_alns"] > 0


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = tmp_path_factory.mktemp("quant_model") / "quant_model_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "thermite_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "quant_model_main.cpp"), "-o", str(exe)])
    return exe


def _run_model(model, tmp_path, data):
    (tmp_path / "in.bin").write_bytes(data)
    p = subprocess.run([str(model), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True)
    return p.returncode, (tmp_path / "out.bin").read_bytes() if p.returncode == 0 else p.stderr


def _model_tables(t, out):
    n_tot, n_g = 8 * len(qc.TOTAL_NAMES), 32 * len(t["genes"])
    tot = np.frombuffer(out[:n_tot], "<u8")
    return dict(totals={k: int(v) for k, v in zip(qc.TOTAL_NAMES, tot)}, genes=np.frombuffer(out[n_tot: n_tot + n_g], qc.GENE_DT),
                junctions=np.frombuffer(out[n_tot + n_g:], qc.JUNCTION_DT))


SHAPES = ["empty", "no_alignments", "one_read_5000", "unique_70000", "forty_introns", "long_run", "both_strands", "later_overhang"]


@pytest.mark.parametrize("name", SHAPES)
def test_model_gives_the_expected_tables_on_the_shapes(model, tmp_path, name):
    if "syn_t" not in _memo:
        _memo["syn_t"] = qc.syn_tables()
    t = _memo["syn_t"]
    exp = None
    for k, view in enumerate(qc.shape_cases(t)[name]):
        rc, out = _run_model(model, tmp_path, qc.model_input(t, *view))
        assert rc == 0, out
        one = qc.expected_tables(t, *view)
        qc.assert_tables_equal(_model_tables(t, out), one, "%s view %d" % (name, k))
        exp = one if exp is None else qc.add_tables(exp, one)
    qc.check_invariants(exp)
    if name == "forty_introns":
        assert exp["totals"]["n_junction_hits"] == 3 * 41 and int(exp["junctions"]["max_overhang"].min()) == 0
    if name == "both_strands":
        assert len(exp["junctions"]) == 2 and exp["junctions"]["strand"].tolist() == [1, 0] and exp["junctions"]["n_unique"].tolist() == [1, 2]
    if name == "later_overhang":
        assert len(exp["junctions"]) == 1 and int(exp["junctions"]["max_overhang"][0]) == 15 and int(exp["junctions"]["n_unique"][0]) == 3
    if name == "long_run":
        assert exp["totals"]["n_long_run_alns"] == 1 and exp["totals"]["n_spliced_alns"] == 1


def test_model_on_the_big_gene_table(model, tmp_path):
    t = qc.big_gene_tables()
    view = qc.big_gene_view(t)
    rc, out = _run_model(model, tmp_path, qc.model_input(t, *view))
    assert rc == 0, out
    exp = qc.expected_tables(t, *view)
    qc.assert_tables_equal(_model_tables(t, out), exp)
    g = exp["genes"]["exonic_unique"] + exp["genes"]["exonic_multi"]
    assert len(g) == 12000 and g.min() >= 1 and int(g.sum()) == 32000


def test_model_on_the_oracle_of_the_synthetic_run(model, tmp_path):
    t, r = _syn()
    dig, words = cc.expected_alignments(r.alns, r.ops)
    rc, out = _run_model(model, tmp_path, qc.model_input(t, r.offsets, r.alns, dig, words))
    assert rc == 0, out
    qc.assert_tables_equal(_model_tables(t, out), qc.from_oracle(t, r))


def test_model_refuses_an_index_out_of_range(model, tmp_path):
    t = _syn()[0]
    off, alns, dig, words = qc.shape_cases(t)["both_strands"][0]
    alns = alns.copy()
    alns["tx_or_gene_idx"][1] = len(t["txs"])
    assert _run_model(model, tmp_path, qc.model_input(t, off, alns, dig, words))[0] == 3
