"""CPU side of the cell-by-gene UMI matrix (include/thermite_io.h: thm_cells): the ABI, the tag rules of
tests/cells_common.py against cases decided by hand, the functions the kernels spread over threads
(thermite_amd/csrc/cells_device.h) run serially by tests/cpp/cells_model_main.cpp -- a stand-alone program under
AddressSanitizer and UBSan, its name pool allocated to the byte -- against that expectation, and the synthetic run's
coverage conditions."""
import ctypes
import os
import re
import subprocess

import pytest

import cells_common as cl
import quant_common as qc
from oracle import pyoracle as orc
from thermite_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["thm_cells_create", "thm_cells_free", "thm_cells_add", "thm_cells_add_view", "thm_cells_fetch", "thm_cells_reset"]
SYN_SEED = 2024
INTRONIC = capi.CELLS_INTRONIC   # (the binding under test: without it nothing here is collected)
_memo = {}


def _syn():
    """(tables, oracle result, names) of the synthetic run, once"""
    if "syn" not in _memo:
        t = qc.syn_tables()
        bases, off = qc.syn_reads(t)
        r = orc.Index(t).align_batch(bases, off, capi.CI_OPTS, n_threads=8)
        assert r.counters[15] == 0
        _memo["syn"] = (t, r, cl.gen_names(len(off) - 1, SYN_SEED))
    return _memo["syn"]


# ------------------------------------------------------------------ ABI
def test_abi_symbols_and_layouts(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "thermite_io.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in capi.IO_ABI_SYMBOLS and hasattr(capi.lib(), s), s
    structs = [("thm_cells_totals", capi.CellsTotals), ("thm_cells_info", capi.CellsInfo), ("thm_cells_view", capi.CellsView)]
    body = ""
    for name, cls in structs:
        body += '  printf(" %%zu", sizeof(%s));\n' % name
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (name, f) for f, _ in cls._fields_)
    body += '  printf(" %zu %zu", sizeof(thm_cell), sizeof(thm_cell_entry));\n'
    body += "".join('  printf(" %%zu", offsetof(thm_cell, %s));\n' % f for f in cl.CELL_DT.names)
    body += "".join('  printf(" %%zu", offsetof(thm_cell_entry, %s));\n' % f for f in cl.ENTRY_DT.names)
    body += '  printf(" %u %u", THM_CELLS_INTRONIC, THM_CELLS_MAX_LEN);\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "thermite_io.h"\nint main(void) {\n' + body + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True).stdout.split()]
    want = []
    for _, cls in structs:
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    want += [24, 16] + [cl.CELL_DT.fields[f][1] for f in cl.CELL_DT.names] + [cl.ENTRY_DT.fields[f][1] for f in cl.ENTRY_DT.names]
    want += [capi.CELLS_INTRONIC, capi.CELLS_MAX_LEN]
    assert got == want
    assert ctypes.sizeof(capi.CellsTotals) == 64 and [f for f, _ in capi.CellsTotals._fields_] == cl.TOTAL_NAMES
    assert capi.CELL_DT == cl.CELL_DT and capi.CELL_ENTRY_DT == cl.ENTRY_DT
    assert issubclass(capi.Cells, capi._RunSummary)
    for knob in ("THM_CELLS=1", "THM_CELLS_CB_LEN", "THM_CELLS_UMI_LEN", "THM_CELLS_MIN_UMIS"):
        assert knob in hdr, knob


def test_null_arguments_need_no_device():
    L = capi.lib()
    h, info, view, cv = ctypes.c_void_p(), capi.CellsInfo(), capi.CellsView(), capi.CigarView()
    assert L.thm_cells_create(None, 0, 16, 12, 0, ctypes.byref(h)) == capi.ERR_INVALID_ARG and not h
    assert L.thm_cells_create(None, 0, 16, 12, 0, None) == capi.ERR_INVALID_ARG
    assert L.thm_cells_add(None, ctypes.byref(info)) == capi.ERR_INVALID_ARG
    assert L.thm_cells_add_view(None, ctypes.byref(cv), None, None, ctypes.byref(info)) == capi.ERR_INVALID_ARG
    assert L.thm_cells_fetch(None, 1, ctypes.byref(view)) == capi.ERR_INVALID_ARG
    assert L.thm_cells_reset(None) == capi.ERR_INVALID_ARG
    L.thm_cells_free(None)


# ------------------------------------------------------------------ the tag, by hand
def test_the_expectations_tag_rules_on_cases_decided_by_hand():
    assert cl.pack(b"A") == 0 and cl.pack(b"T") == 3 and cl.pack(b"CA") == 4 and cl.pack(b"ACGT") == 0b00011011
    assert cl.pack(b"T" * 16) == 0xFFFFFFFF and cl.pack(b"ACGN") is None and cl.pack(b"acgt") is None
    assert cl.unpack(0b00011011, 4) == "ACGT" and cl.unpack(0, 16) == "A" * 16
    # integer order is lexicographic order
    seqs = [b"AAAC", b"AACA", b"ACAA", b"CAAA", b"GTTT", b"TAAA"]
    assert [cl.pack(s) for s in seqs] == sorted(cl.pack(s) for s in seqs)
    assert cl.parse_tag(b"r1_ACGT_TG", 4, 2) == (0b00011011, 0b1110)
    assert cl.parse_tag(b"r1_ACGT_TG extra_AAAA_CC", 4, 2) == (0b00011011, 0b1110)
    assert cl.parse_tag(b"_ACGT_TG", 4, 2) == (0b00011011, 0b1110)
    assert cl.parse_tag(b"ACGT_TG", 4, 2) is None
    assert cl.parse_tag(b"r1 x_ACGT_TG", 4, 2) is None
    assert cl.parse_tag(b"r1_ACGT-TG", 4, 2) is None and cl.parse_tag(b"r1_ACNT_TG", 4, 2) is None and cl.parse_tag(b"r1_ACGT_Tg", 4, 2) is None
    assert cl.parse_tag(b"", 1, 1) is None and cl.parse_tag(b"_A_C", 1, 1) == (0, 1)
    for cb, umi in ((1, 1), (16, 16), (16, 12), (5, 3)):
        for name, tagged in cl.tag_cases(cb, umi):
            assert (cl.parse_tag(name, cb, umi) is not None) == tagged, (cb, umi, name)


def test_rows_of_a_small_molecule_dict_by_hand():
    mol = {(5, 2, 0): 3, (5, 2, 1): 1, (5, 0, 1): 2, (1, 7, 9): 4, (9, 1, 1): 1, (9, 1, 2): 1}
    cells, entries, counts = cl.rows(mol, 1)
    assert [tuple(int(x) for x in c) for c in cells] == [(4, 1, 1, 1, 0), (6, 5, 3, 2, 0), (2, 9, 2, 1, 0)]
    assert [tuple(int(x) for x in e) for e in entries] == [(0, 7, 1, 4), (1, 0, 1, 2), (1, 2, 2, 4), (2, 1, 2, 2)]
    assert counts == dict(n_molecules=6, n_barcodes=3, n_cells_below=0)
    cells, entries, counts = cl.rows(mol, 2)
    assert [int(c["barcode"]) for c in cells] == [5, 9] and [tuple(int(x) for x in e) for e in entries] == [(0, 0, 1, 2), (0, 2, 2, 4), (1, 1, 2, 2)]
    assert counts["n_cells_below"] == 1
    t = dict(genes=[0] * 8, gene_ids=["G%d" % g for g in range(8)], gene_names=["n%d" % g for g in range(8)])
    mtx, barcodes, features = cl.mtx_of(t, cells, entries, 2)
    assert mtx == "%%MatrixMarket matrix coordinate integer general\n8 2 3\n1 1 1\n3 1 2\n2 2 2\n"
    assert barcodes == "CC\nGC\n" and features.splitlines()[2] == "G2\tn2\tGene Expression"


# ------------------------------------------------------------------ the synthetic run holds what it is meant to test
def test_coverage_conditions_of_the_synthetic_run():
    t, r, names = _syn()
    pool, name_off = cl.join_names(names)
    for flags in (0, cl.INTRONIC_FLAG):
        mol, tot = cl.expected(t, r.offsets, r.alns, None, pool, name_off, flags, 16, 12)
        cl.check_invariants(tot, mol)
        assert max(mol.values()) >= 3                                  # some molecule has three reads or more
        cells, entries, counts = cl.rows(mol, 1)
        assert int(entries["n_umis"].max()) >= 2 and int(cells["n_genes"].max()) >= 2
        by_bc_umi = {}
        for bc, gene, umi in mol:
            by_bc_umi.setdefault((bc, umi), set()).add(gene)
        assert any(len(g) >= 2 for g in by_bc_umi.values())           # one (barcode, UMI) occurs with two genes
        for k in ("n_counted_reads", "n_untagged_reads", "n_multi_reads", "n_unmapped_reads"):
            assert tot[k] > 0, k
        kept = cl.rows(mol, 3)
        assert 0 < len(kept[0]) < len(cells) and kept[2]["n_cells_below"] == len(cells) - len(kept[0])
        if flags:
            assert tot["n_intronic_skipped_reads"] == 0 and tot["n_counted_reads"] > plain["n_counted_reads"]
        else:
            assert tot["n_intronic_skipped_reads"] > 0 and tot["n_intergenic_reads"] > 0
            plain = tot


# ------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cells_model") / "cells_model_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "thermite_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "cells_model_main.cpp"), "-o", str(exe)])
    return exe


def _run_model(model, tmp_path, data):
    (tmp_path / "in.bin").write_bytes(data)
    p = subprocess.run([str(model), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True)
    return p.returncode, (tmp_path / "out.bin").read_bytes() if p.returncode == 0 else p.stderr


def _check_model(model, tmp_path, t, offsets, alns, status, names, flags, cb_len, umi_len, min_umis):
    pool, name_off = cl.join_names(names)
    rc, out = _run_model(model, tmp_path, cl.model_input(t, offsets, alns, status, pool, name_off, flags, cb_len, umi_len, min_umis))
    assert rc == 0, out
    mol, tot = cl.expected(t, offsets, alns, status, pool, name_off, flags, cb_len, umi_len)
    got_tot, counts, cells, entries, rows = cl.model_output(out)
    exp_cells, exp_entries, exp_counts = cl.rows(mol, min_umis)
    assert got_tot == tot and counts == exp_counts
    assert rows == [(k[0], k[1], k[2], mol[k]) for k in sorted(mol)]
    assert cl.pack_rows(cells, entries) == cl.pack_rows(exp_cells, exp_entries)
    return mol, tot


@pytest.mark.parametrize("cb_len,umi_len", [(1, 1), (16, 16), (16, 12), (5, 3)])
def test_model_on_the_tag_cases(model, tmp_path, cb_len, umi_len):
    if "syn_t" not in _memo:
        _memo["syn_t"] = qc.syn_tables()
    t = _memo["syn_t"]
    cases = cl.tag_cases(cb_len, umi_len)
    names = [c[0] for c in cases]
    assert cases[-1][1] and not names[-1].endswith(b" ")   # the name that ends the pool carries a tag up to the pool's last byte
    view = qc.uniform_view(len(names), 1, 0, 1000, 3, [(91, "M")])
    mol, tot = _check_model(model, tmp_path, t, view[0], view[1], None, names, 0, cb_len, umi_len, 1)
    assert tot["n_counted_reads"] == sum(1 for c in cases if c[1]) and tot["n_untagged_reads"] == sum(1 for c in cases if not c[1])
    assert len(mol) == 1   # every tagged case carries the same barcode and UMI: the comment's tag was ignored
    # each name alone, as the whole pool: the first and the last byte of the pool are the name's
    for name, tagged in cases:
        one = qc.uniform_view(1, 1, 0, 1000, 3, [(91, "M")])
        _, tot = _check_model(model, tmp_path, t, one[0], one[1], None, [name], 0, cb_len, umi_len, 1)
        assert tot["n_counted_reads"] == (1 if tagged else 0), name


def test_model_on_every_class_of_read(model, tmp_path):
    t = qc.big_gene_tables()
    offsets, alns, status, names, _ = cl.class_view(t, 16, 12)
    for flags in (0, cl.INTRONIC_FLAG):
        mol, tot = _check_model(model, tmp_path, t, offsets, alns, status, names, flags, 16, 12, 1)
        assert all(tot[k] > 0 for k in cl.TOTAL_NAMES if k != "n_intronic_skipped_reads" or not flags), tot
        assert max(k[1] for k in mol) == len(t["genes"]) - 1 >= 8192   # the gene field of the key is wide
    _check_model(model, tmp_path, t, offsets, alns, status, names, 1, 16, 12, 2)


def test_model_on_the_oracle_of_the_synthetic_run(model, tmp_path):
    t, r, names = _syn()
    for flags, min_umis in ((0, 1), (cl.INTRONIC_FLAG, 3)):
        _check_model(model, tmp_path, t, r.offsets, r.alns, None, names, flags, 16, 12, min_umis)


def test_model_refuses_an_index_out_of_range(model, tmp_path):
    t = _syn()[0]
    view = qc.uniform_view(3, 1, 0, 1000, 3, [(91, "M")])
    alns = view[1].copy()
    alns["tx_or_gene_idx"][1] = len(t["txs"])
    pool, name_off = cl.join_names([b"a_A_C"] * 3)
    assert _run_model(model, tmp_path, cl.model_input(t, view[0], alns, None, pool, name_off, 0, 1, 1, 1))[0] == 3
