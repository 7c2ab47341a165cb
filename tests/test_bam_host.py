"""CPU side of the device BAM encoder (include/thermite_io.h: thm_bam_view and the calls around it): the ABI, the
host call thm_writer_wrap_bam against the oracle's record stream, the committed golden record file, and -- by the
oracle alone -- what the read sets of tests/test_gpu_bam.py contain, so that byte equality there is not vacuous."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bam_common as bc
from oracle import aln_writer as ow
from oracle import pyoracle as orc
from thermite_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["thm_batch_upload_reads", "thm_batch_fetch_bam", "thm_align_batch_bam", "thm_writer_wrap_bam"]
_cache = {}


def _oracle(name):
    """(tables, read set, oracle result, record bytes, per-read byte offsets) of a read set"""
    if name not in _cache:
        t = bc.tables(bc.REF_OF[name])
        rs = bc.read_set(name, t)
        b = bc.batch_of(rs)
        r = orc.Index(t).align_batch(b["bases"], b["offsets"], rs["opts"], n_threads=8)
        assert r.counters[15] == 0
        data, off = bc.oracle_records(t, rs, r)
        _cache[name] = (t, rs, r, data, off)
    return _cache[name]


# ------------------------------------------------------------------ ABI
def test_abi_symbols_and_view_layout(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "thermite_io.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in capi.IO_ABI_SYMBOLS
        assert hasattr(capi.lib(), s), "missing export: " + s
    assert "THM_T_BAM = 6" in open(os.path.join(ROOT, "include", "thermite.h")).read() and capi.TIMING_NAMES[6] == "bam"
    # the C compiler's layout of thm_bam_view against the ctypes structure
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "thermite_io.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(thm_bam_view));\n' +
                   "".join('  printf(" %%zu", offsetof(thm_bam_view, %s));\n' % f for f, _ in capi.BamView._fields_) +
                   '  printf(" %u\\n", THM_BAM_NO_ANNOTATION_TAGS);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True).stdout.split()]
    want = [ctypes.sizeof(capi.BamView)] + [getattr(capi.BamView, f).offset for f, _ in capi.BamView._fields_] + [capi.BAM_NO_ANNOTATION_TAGS]
    assert got == want and ctypes.sizeof(capi.BamView) == 56


def test_cpp_header_has_the_record_calls(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "thermite.hpp"\n'
                   "auto p1 = &thermite::Aligner::align_reads_bam;\n"
                   "auto p2 = &thermite::ThermiteAligner::align_read_records;\n"
                   "auto p3 = &thermite::ThermiteAligner::align_read_records_with_tags;\nint main() { return 0; }\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "bam_main.cpp")])


# ------------------------------------------------------------------ thm_writer_wrap_bam
class _Records:
    def __init__(self, data, off):
        self.data, self.read_rec_off, self.n_records = np.frombuffer(data, np.uint8), off, 0


_WRAP_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_bam_host as me
me.wrap_check(%r)
print("wrap ok")
"""


def wrap_check(name):
    t, rs, r, data, off = _oracle(name)
    ix = capi.Index(t)
    quals = rs["quals"] if rs["quals"] is not None else [b""] * len(rs["seqs"])
    want = ow.bam_stream(t, rs["names"], rs["seqs"], quals, r)
    for threads in (1, 4):
        w = capi.Writer(ix, capi.FMT_BAM, n_threads=threads)
        out = w.wrap_bam(_Records(data, off))
        assert ow.bgzf_decompress(w.header() + out + w.trailer()) == want, (name, threads)
        # the host encoder's own blocks for the same reads: equal even before inflation (same ranges, same deflate)
        full = capi.BatchResult.__new__(capi.BatchResult)
        full.offsets, full.alns, full.ops = r.offsets, r.alns, r.ops
        assert w.format_batch(bc.batch_of(rs), full) == out, (name, threads)
        w.close()
    ix.close()


@pytest.mark.parametrize("level", [None, "1"], ids=["own-deflate", "zlib-1"])
def test_wrap_bam_inflates_to_the_oracle_stream(level):
    """1 and 4 threads, THM_BAM_LEVEL unset and 1 (read once per process: a child each); syn has more than 4096 reads,
    so four threads really cut it"""
    env = dict(os.environ)
    env.pop("THM_BAM_LEVEL", None)
    if level is not None:
        env["THM_BAM_LEVEL"] = level
    for name in ("test_query", "syn", "micro"):
        out = subprocess.run([sys.executable, "-c", _WRAP_CHILD % (ROOT, os.path.join(ROOT, "tests"), name)], env=env,
                             capture_output=True, text=True)
        assert out.returncode == 0 and "wrap ok" in out.stdout, out.stderr[-2000:]


def test_wrap_bam_argument_errors():
    t, rs, r, data, off = _oracle("test_query")
    ix = capi.Index(t)
    w = capi.Writer(ix, capi.FMT_BAM, n_threads=2)

    def code(d, o):
        with pytest.raises(capi.ThermiteError) as e:
            w.wrap_bam(_Records(d, np.array(o, "<u8")))
        assert "thm_writer_wrap_bam" in str(e.value)
        return e.value.code

    o = off.copy()
    o[0] = 1
    assert code(data, o) == capi.ERR_INVALID_ARG          # does not start at 0
    o = off.copy()
    o[-1] -= 1
    assert code(data, o) == capi.ERR_INVALID_ARG          # does not end at n_bytes
    o = off.copy()
    o[3], o[4] = o[4], o[3] - 1
    assert code(data, o) == capi.ERR_INVALID_ARG          # descends
    assert w.wrap_bam(_Records(data, off))                # (the writer still works)
    assert w.wrap_bam(_Records(b"", np.zeros(1, "<u8"))) == b""   # no reads: no blocks
    v = capi.BamView(0, 0, 0, None, None, 0, None)
    assert capi.lib().thm_writer_wrap_bam(w.h, ctypes.byref(v), ctypes.byref(capi.Text())) == capi.ERR_INVALID_ARG
    assert capi.lib().thm_writer_wrap_bam(w.h, None, ctypes.byref(capi.Text())) == capi.ERR_INVALID_ARG
    w.close()
    sam = capi.Writer(ix, capi.FMT_SAM)
    with pytest.raises(capi.ThermiteError) as e:
        sam.wrap_bam(_Records(data, off))
    assert e.value.code == capi.ERR_INVALID_ARG and "not a BAM writer" in str(e.value)
    sam.close()
    ix.close()


# ------------------------------------------------------------------ golden file
def test_golden_record_file_is_the_oracles():
    t, rs, r, data, off = _oracle("test_query")
    assert open(bc.GOLDEN_BIN, "rb").read() == data
    assert len(bc.split_records(data)) == 11 and len(off) == 11


# ------------------------------------------------------------------ what the read sets contain
def test_read_sets_cover_the_encoder():
    """Every condition the device encoder has a rule for occurs in the oracle's records of the read sets the GPU tests
    use.  (The issue names "a TX:Z with at least 65 N runs": TX:Z carries the transcript's CIGAR, which has no N -- the
    introns are in the genome CIGAR of the same record.  Pinned here: an exonic record, TX:Z present, whose CIGAR has
    at least 65 N words, and a TX:Z CIGAR text of more than one run.)"""
    seen = set()
    for name in bc.READ_SETS:
        t, rs, r, data, off = _oracle(name)
        recs = [bc.parse_record(x) for x in bc.split_records(data)]
        assert len(recs) == int(np.maximum(np.diff(r.offsets.astype(np.int64)), 1).sum())
        if rs["quals"] is None:
            seen.add("no qualities")
            assert all(x["qual"] == b"\xff" * x["l_seq"] for x in recs)
        if any(b" " in n for n in rs["names"]):
            seen.add("name with a space")
            assert all(b" " not in x["qname"] for x in recs)
        if any(re.search(b"[acgt]", s) for s in rs["seqs"]) and any(b"N" in s for s in rs["seqs"]):
            seen.add("lowercase and N bases")
        for x in recs:
            aux = {tag: (ty, v) for tag, ty, v, _ in x["aux"]}
            if x["flag"] & 4:
                seen.add("unmapped")
                assert (x["ref_id"], x["pos"], x["mapq"], x["bin"], x["aux"], x["cigar"]) == (-1, -1, 255, 4680, [], ())
                continue
            if x["flag"] & 16:
                seen.add("reverse strand")
            if x["flag"] & 256:
                seen.add("secondary")
            if x["l_seq"] % 2:
                seen.add("odd length")
            else:
                seen.add("even length")
            seen.add("RE:" + aux[b"RE"][1].decode())
            nh = int.from_bytes(aux[b"NH"][1], "little")
            seen.add("NH %s" % (nh if nh < 5 else ">=5"))
            assert x["mapq"] == {1: 255, 2: 3, 3: 2, 4: 1}.get(nh, 0)
            if aux[b"NH"][0] == b"S" or aux[b"HI"][0] == b"S":
                seen.add("tag type S")
            n_runs = sum(1 for w in x["cigar"] if (w & 15) == 3)
            if b"TX" in aux:
                if n_runs >= 65:
                    seen.add("exonic record with >= 65 N words")
                if len(re.findall(rb"\d+[MIDS]", aux[b"TX"][1].split(b",")[2])) > 1:
                    seen.add("TX:Z CIGAR of several runs")
    want = {"no qualities", "name with a space", "lowercase and N bases", "unmapped", "reverse strand", "secondary", "odd length",
            "even length", "RE:E", "RE:N", "RE:I", "NH 1", "NH 2", "NH 3", "NH 4", "NH >=5", "tag type S",
            "exonic record with >= 65 N words", "TX:Z CIGAR of several runs"}
    assert want <= seen, sorted(want - seen)


def test_strip_annotation_parser():
    """the aux parser of bam_common.py removes exactly TX GX GN RE and keeps AS NH HI nM"""
    t, rs, r, data, off = _oracle("multi")
    stripped = bc.strip_annotation(data)
    a, b = bc.split_records(data), bc.split_records(stripped)
    assert len(a) == len(b) and len(stripped) < len(data)
    for x, y in zip(a, b):
        px, py = bc.parse_record(x), bc.parse_record(y)
        assert [f[0] for f in py["aux"]] == [f[0] for f in px["aux"] if f[0] not in bc.ANNOTATION_TAGS]
        assert x[4: px["aux_at"]] == y[4: py["aux_at"]]
        if not (px["flag"] & 4):
            assert [f[0] for f in py["aux"]] == [b"AS", b"NH", b"HI", b"nM"]
