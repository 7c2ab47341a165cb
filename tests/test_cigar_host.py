"""CPU: the CIGAR surface of the C ABI (thm_aln_digest, thm_cigar_view, thm_batch_fetch_cigars,
thm_align_batch_cigars, thm_cigar_encode_batch, thm_writer_format_batch_cigars) is exported and laid out as the
header says; the Python restatement the GPU tests compare against (tests/cigar_common.py) is pinned by the committed
SAM / PAF goldens; argument errors that need no device."""
import ctypes
import os
import subprocess

import numpy as np

import cigar_common as cc
from oracle import pyoracle as orc
from thermite_amd import capi, refdata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["thm_batch_fetch_cigars", "thm_align_batch_cigars", "thm_cigar_encode_batch", "thm_writer_format_batch_cigars"]


def test_library_exports_the_cigar_entry_points():
    L = ctypes.CDLL(capi.SO_PATH)
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), "missing export: " + s
    assert set(NEW_SYMBOLS[:3]) <= set(capi.ABI_SYMBOLS) and NEW_SYMBOLS[3] in capi.IO_ABI_SYMBOLS


def test_struct_layouts_match_a_c99_compile_of_the_header(tmp_path):
    """sizeof / offsetof of thm_aln_digest and thm_cigar_view as a C compiler sees include/thermite.h, against the
    ctypes structures and the numpy record of the binding"""
    structs = {"thm_aln_digest": capi.AlnDigest, "thm_cigar_view": capi.CigarView}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "thermite_io.h"', "int main(void) {"]
    for name, st in structs.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for f, _ in st._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f))
    lines.append('  printf("flags %u %u %d %d\\n", THM_DIGEST_LONG_RUN, THM_DIGEST_MALFORMED, (int)THM_T_CIGAR, (int)THM_N_TIMINGS);')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe)])
    got = dict(l.split(" ", 1) for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for name, st in structs.items():
        assert int(got[name]) == ctypes.sizeof(st), name
        for f, _ in st._fields_:
            assert int(got["%s.%s" % (name, f)]) == getattr(st, f).offset, (name, f)
    assert ctypes.sizeof(capi.AlnDigest) == 40 == capi.DIGEST_DT.itemsize == cc.DIGEST_DT.itemsize
    for f, _ in capi.AlnDigest._fields_:
        assert capi.DIGEST_DT.fields[f][1] == getattr(capi.AlnDigest, f).offset == cc.DIGEST_DT.fields[f][1]
    assert got["flags"] == "%d %d 5 8" % (capi.DIGEST_LONG_RUN, capi.DIGEST_MALFORMED)
    assert (cc.LONG_RUN, cc.MALFORMED) == (capi.DIGEST_LONG_RUN, capi.DIGEST_MALFORMED)
    assert capi.TIMING_NAMES[5] == "cigar" and capi.N_TIMINGS == 8


def _test_query(data_dir):
    t = refdata.load_reference(data_dir + "/test_ref.fasta", data_dir + "/test_ref.gtf")
    names, seqs, quals = refdata.parse_fastq(data_dir + "/test_query.fastq")
    bases, off = refdata.pack_reads(seqs)
    res = orc.Index(t).align_batch(bases, off, dict(capi.DEFAULT_OPTS, min_seed_len=3, min_aln_score=0))
    return t, names, seqs, res


def test_restatement_is_pinned_by_the_sam_golden(data_dir, golden_dir):
    """CIGAR column, nM and the TX:Z CIGAR of every record of tests/golden/test_query.sam"""
    t, names, seqs, res = _test_query(data_dir)
    dig, words = cc.expected_alignments(res.alns, res.ops)
    recs = [l.split("\t") for l in open(os.path.join(golden_dir, "test_query.sam")).read().splitlines() if not l.startswith("@")]
    mapped = [r for r in recs if not int(r[1]) & 4]
    assert len(mapped) == len(res.alns) > 0
    for i, r in enumerate(mapped):
        d = dig[i]
        o = int(d["cigar_off"])
        assert cc.words_to_text(words[o: o + int(d["n_cigar"])]) == r[5], (i, r[0])
        tags = dict((x[:4], x[5:]) for x in r[11:])
        assert int(tags["nM:i"]) == int(d["n_subst"]), (i, r[0])
        assert d["flags"] == 0
        if "TX:Z" in tags:
            assert res.alns[i]["aln_type"] == 0
            assert cc.words_to_text(words[o + int(d["n_cigar"]): o + int(d["n_cigar"]) + int(d["n_tx_cigar"])]) == tags["TX:Z"].split(",")[2]
        else:
            assert d["n_tx_cigar"] == 0
        assert int(d["ref_len"]) == sum(n for n, k in cc.cigar_runs(r[5]) if k in "MDN")
    assert int(dig["cigar_off"][-1]) + int(dig["n_cigar"][-1]) + int(dig["n_tx_cigar"][-1]) == len(words)


def test_restatement_is_pinned_by_the_paf_golden(data_dir, golden_dir):
    """columns 10 and 11 (matches, matches + gaps) of every record of tests/golden/test_query.paf"""
    t, names, seqs, res = _test_query(data_dir)
    dig, _ = cc.expected_alignments(res.alns, res.ops)
    recs = [l.split("\t") for l in open(os.path.join(golden_dir, "test_query.paf")).read().splitlines()]
    assert len(recs) == len(res.alns)
    for i, r in enumerate(recs):
        assert (int(r[9]), int(r[10])) == (int(dig[i]["n_match"]), int(dig[i]["n_not_yclip"])), (i, r[0])


def test_restatement_on_hand_written_streams():
    e = cc.expected_stream
    assert e(b"") == ([], 0, 0, 0, 0, 0)
    assert e(bytes([0, 1, 0, 0, 1])) == ([5 << 4], 5, 3, 2, 5, 0)                                   # 5M
    assert e(cc.clip(5, 7) + cc.clip(5, 7)) == ([(7 << 4) | 3], 7, 0, 0, 0, 0)                      # equal clips merge: 7N
    assert e(cc.clip(5, 7) + cc.clip(5, 8)) == ([(7 << 4) | 3, (8 << 4) | 3], 15, 0, 0, 0, 0)
    assert e(cc.clip(4, 2) + bytes([0, 2, 3]) + cc.clip(4, 1)) == ([(2 << 4) | 4, 1 << 4, (1 << 4) | 2, (1 << 4) | 1, (1 << 4) | 4], 2, 1, 0, 5, 0)
    assert e(cc.clip(5, 1 << 28))[5] == cc.LONG_RUN and e(cc.clip(5, 1 << 28))[:2] == ([], 1 << 28)
    for bad in (bytes([6]), bytes([0, 4]), bytes([0, 5, 1, 2, 3]), bytes([4, 0, 0, 0, 0, 9])):
        assert e(bad) == ([], 0, 0, 0, 0, cc.MALFORMED), bad
    # payload bytes that look like clip kinds are payload: Xclip(0x04050405), Match
    assert e(bytes([4, 5, 4, 5, 4, 0])) == ([(0x04050405 << 4) | 4, 1 << 4], 1, 1, 0, 2, 0)


def test_argument_errors_need_no_device():
    L = capi.lib()
    v = capi.CigarView()
    off = np.zeros(2, "<u8")
    assert L.thm_batch_fetch_cigars(None, ctypes.byref(v)) == capi.ERR_INVALID_ARG
    assert L.thm_batch_fetch_cigars(None, None) == capi.ERR_INVALID_ARG
    assert L.thm_align_batch_cigars(None, None, off.ctypes.data, 1, ctypes.byref(v)) == capi.ERR_INVALID_ARG
    assert L.thm_cigar_encode_batch(None, None, off.ctypes.data, 1, ctypes.byref(v)) == capi.ERR_INVALID_ARG
    assert L.thm_cigar_encode_batch(None, None, None, 0, None) == capi.ERR_INVALID_ARG
    t = capi.Text()
    rb = capi.ReadBatch()
    assert L.thm_writer_format_batch_cigars(None, ctypes.byref(rb), ctypes.byref(v), ctypes.byref(t)) == capi.ERR_INVALID_ARG


def test_writer_rejects_inconsistent_cigar_views(data_dir):
    """the writer is host code: a view whose digests point outside the word pool, or carry a flag, is refused"""
    t, names, seqs, res = _test_query(data_dir)
    ix = capi.Index(t)
    dig, words = cc.expected_alignments(res.alns, res.ops)
    batch = dict(bases=np.concatenate([np.frombuffer(bytes(s), np.uint8) for s in seqs]), offsets=res.offsets * 0, quals=None,
                 names=np.frombuffer(b"".join(n.encode() for n in names), np.uint8),
                 name_off=np.cumsum([0] + [len(n) for n in names]).astype("<u8"))
    batch["offsets"] = np.cumsum([0] + [len(s) for s in seqs]).astype("<u8")

    class R:
        pass

    def result(d, w):
        r = R()
        r.offsets, r.alns, r.digests, r.cigar = res.offsets, res.alns, np.ascontiguousarray(d), np.ascontiguousarray(w, "<u4")
        return r

    for fmt in (capi.FMT_SAM, capi.FMT_PAF, capi.FMT_BAM):
        w = capi.Writer(ix, fmt, n_threads=2)
        full = w.format_batch(batch, res)
        assert w.format_batch_cigars(batch, result(dig, words)) == full, fmt   # host-only: restated digests render alike
        for spoil in ("range", "flag"):
            d = dig.copy()
            if spoil == "range":
                d["cigar_off"][-1] = len(words)
            else:
                d["flags"][0] = capi.DIGEST_LONG_RUN
            try:
                w.format_batch_cigars(batch, result(d, words))
                raise AssertionError("accepted a digest with a bad " + spoil)
            except capi.ThermiteError as e:
                assert e.code == capi.ERR_INTERNAL
        w.close()
    ix.close()
