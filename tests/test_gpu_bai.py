"""-m gpu: the BAI index of a coordinate-sorted run built on the device (kernels_bai.hip, thm_bam_sorter_index).  Every
case compares bytes with the serial walk of tests/bai_common.py over the inflated members the sorter handed out, the
view's counts with the parsed index, and region queries through the returned index over the assembled file with a walk
of the whole stream."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import bai_common as xc
import bam_common as bc
import bam_sort_common as sc
import bgzf_common as zc
from gpu_common import World
from thermite_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = sc.BLOCK_IN
N_SQ = 4
ODD_FIRST = 2 ** 32 + 12345
_worlds, _cases = {}, {}


def _world(key):
    if key not in _worlds:
        _worlds[key] = World(bc.tables(key))
    return _worlds[key]


def _case(name):
    if not _cases:
        _cases.update(xc.synthetic_cases(N_SQ))
    return _cases[name]


def _header(w):
    wr = capi.Writer(w.ix, capi.FMT_BAM)
    out = wr.header_sorted(), wr.trailer()
    wr.close()
    return out


def _drain(s, window=0):
    """the rest of the sorted stream as BGZF windows -> (the members back to back, their sizes, the inflated stream)"""
    data, sizes, raw = [], [], []
    for v in s.windows(window):
        raw.append(zc.check_blocks(v.data, v.block_off)[0])
        sizes += np.diff(v.block_off.astype(np.int64)).tolist()
        data.append(v.data.tobytes())
    return b"".join(data), sizes, b"".join(raw)


def _check(s, w, members, sizes, stream, n_sq, regions=None):
    """the index for the file header + members + trailer: the bytes, the counts, the queries -> the parsed index"""
    header, trailer = _header(w)
    data, info = s.index(len(header))
    assert data == xc.expected_bai(stream, n_sq, sizes, len(header))
    index = xc.parse_bai(data)
    want = xc.counts(index)
    assert {k: info[k] for k in want} == want and info["n_bytes"] == len(data) and info["index_ms"] >= 0
    xc.check_queries(index, header + members + trailer, stream, n_sq, regions)
    return index


def _sorter_of(a, data):
    s = capi.BamSorter(a)
    s.add_records(data)
    s.finish()
    return s


# ------------------------------------------------------------------ 1. the synthetic cases
@pytest.mark.parametrize("name", ["empty", "one_reference", "bin_levels", "no_span", "linear", "merge", "member_cuts", "many"])
def test_synthetic_records(name):
    w = _world("test_ref")
    data = _case(name)
    s = _sorter_of(w.a, data)
    members, sizes, stream = _drain(s)
    assert stream == sc.sorted_stream(data, N_SQ)
    regions = xc.regions_of(stream, N_SQ)
    index = _check(s, w, members, sizes, stream, N_SQ, regions[::3] if name == "many" else regions)
    if name == "empty":
        assert xc.index_bytes(index) == b"BAI\1" + struct.pack("<I", 4) + bytes(32) + bytes(8)
    if name == "member_cuts":
        assert len(stream) % B == 0 and index["refs"][3]["pseudo"][0][1] == (len(_header(w)[0]) + len(members)) << 16
    if name == "merge":
        parent = xc.reg2bin(5 * xc.W - 30, 5 * xc.W + 20)
        assert [len(dict(r["bins"])[parent]) for r in index["refs"][:2]] == [1, 4]
    s.close()


# ------------------------------------------------------------------ 2. windows and the first member's offset
def test_windows_and_first_member_offset_do_not_show():
    w = _world("test_ref")
    data = _case("member_cuts") + _case("bin_levels")
    got = {}
    for window in (B, 3 * B, 0):
        s = _sorter_of(w.a, data)
        members, sizes, stream = _drain(s, window)
        for first in (0, ODD_FIRST):
            got[(window, first)] = s.index(first)[0]
            assert got[(window, first)] == xc.expected_bai(stream, N_SQ, sizes, first), (window, first)
        assert s.index(0)[0] == got[(window, 0)]   # again, after another offset
        s.close()
    assert got[(B, 0)] == got[(3 * B, 0)] == got[(0, 0)] and got[(B, ODD_FIRST)] == got[(0, ODD_FIRST)]
    # the two differ in virtual offsets only, and by the offset
    a, b = xc.parse_bai(got[(0, 0)]), xc.parse_bai(got[(0, ODD_FIRST)])
    shift = ODD_FIRST << 16
    for ra, rb in zip(a["refs"], b["refs"]):
        assert [(k, [(x + shift, y + shift) for x, y in c]) for k, c in ra["bins"]] == rb["bins"]
        assert [x + shift for x in ra["ioffset"]] == rb["ioffset"]
        assert (ra["pseudo"] is None) == (rb["pseudo"] is None)
        if ra["pseudo"]:
            assert tuple(x + shift for x in ra["pseudo"][0]) == rb["pseudo"][0] and ra["pseudo"][1] == rb["pseudo"][1]


# ------------------------------------------------------------------ 3. real read sets
def _subset(rs, idx):
    return dict(rs, names=[rs["names"][i] for i in idx], seqs=[rs["seqs"][i] for i in idx],
                quals=None if rs["quals"] is None else [rs["quals"][i] for i in idx])


@pytest.mark.parametrize("name", ["test_query", "multi", "syn", "contigs"])
def test_read_sets(name):
    w = _world(bc.REF_OF[name])
    rs = bc.read_set(name, w.t)
    n_sq = sc.n_sq_of(w.t)
    n = len(rs["seqs"])
    a = w.aligner(rs["opts"])
    s = capi.BamSorter(a)
    n_records = 0
    for part in (range(0, n // 3), range(n // 3, n)):
        a.upload_reads(bc.batch_of(_subset(rs, part)))
        a.run()
        n_records += s.add()["n_records"]
    s.finish()
    members, sizes, stream = _drain(s)
    recs = xc.split_records(stream)
    assert len(recs) == n_records and len({xc.fields(r)[0] for r in recs if xc.fields(r)[0] >= 0}) >= 1
    regions = xc.regions_of(stream, n_sq)
    index = _check(s, w, members, sizes, stream, n_sq, regions if len(recs) < 5000 else regions[::4])
    # every mapped record's own bin field is the bin the index put it in: a chunk of that bin holds its virtual offset
    header = _header(w)[0]
    coff = np.concatenate([[len(header)], len(header) + np.cumsum(sizes)]).astype(np.int64)
    at, n_checked = 0, 0
    for rec in recs:
        ref_id, beg, end, is_mapped = xc.fields(rec)
        if ref_id >= 0 and is_mapped:
            own = struct.unpack_from("<H", rec, 14)[0]
            v = int(coff[at // B]) << 16 | at % B
            assert own == xc.reg2bin(beg, end)
            assert any(cb <= v < ce for cb, ce in dict(index["refs"][ref_id]["bins"])[own]), (ref_id, beg, own)
            n_checked += 1
        at += len(rec)
    assert n_checked > 0
    if name == "contigs":
        # most references are short and some got no record: their sections are there, and empty
        with_records = {xc.fields(r)[0] for r in recs} - {-1}
        assert len(index["refs"]) == n_sq and 30 <= len(with_records) < n_sq
        for k in set(range(n_sq)) - with_records:
            assert index["refs"][k] == dict(bins=[], pseudo=None, ioffset=[]), k
    s.close()
    a.close()


def test_failed_reads_count_in_n_no_coor():
    w = _world("chrm")
    sb, so, _ = synth.simulate_reads(w.t, 200, 91, stream=101)
    seqs = [bytes(sb[so[i]: so[i + 1]]) for i in range(200)]
    seqs.insert(77, b"ACGT" * 17000)  # 68 000 bases: beyond the build limit
    rs = dict(names=[b"f%d x" % i for i in range(201)], seqs=seqs, quals=[b"I" * len(x) for x in seqs], opts=capi.CI_OPTS)
    a = w.aligner(capi.CI_OPTS)
    a.upload_reads(bc.batch_of(rs))
    a.run()
    s = capi.BamSorter(a)
    assert s.add()["n_failed_reads"] == 1
    s.finish()
    members, sizes, stream = _drain(s)
    n_sq = sc.n_sq_of(w.t)
    index = _check(s, w, members, sizes, stream, n_sq)
    last = bc.parse_record(xc.split_records(stream)[-1])
    assert last["qname"] == b"f77" and last["ref_id"] == -1
    assert index["n_no_coor"] == sum(xc.fields(r)[0] < 0 for r in xc.split_records(stream)) >= 1
    s.close()
    a.close()


# ------------------------------------------------------------------ 4. errors
def _raises(call):
    with pytest.raises(capi.ThermiteError) as e:
        call()
    assert e.value.code == capi.ERR_INVALID_ARG and "thm_bam_sorter_index" in str(e.value)
    return str(e.value)


def test_state_errors_leave_the_sorter_usable():
    w = _world("test_ref")
    data = _case("member_cuts")
    s = capi.BamSorter(w.a)
    s.add_records(data)
    assert "finish" in _raises(lambda: s.index(0))
    s.finish()
    assert "exhausted" in _raises(lambda: s.index(0))
    v = s.next(B)
    assert v.n_raw_bytes == B
    assert "exhausted" in _raises(lambda: s.index(0))
    members, sizes, stream = _drain(s)   # still drains: the rest
    whole = zc.check_blocks(v.data, v.block_off)[0] + stream
    assert whole == sc.sorted_stream(data, N_SQ)
    sizes = np.diff(v.block_off.astype(np.int64)).tolist() + sizes
    first, info = s.index(7)
    assert first == xc.expected_bai(whole, N_SQ, sizes, 7)
    assert s.index(7)[0] == first   # twice: the same bytes
    s.close()
    # a raw window: no member sizes
    s = _sorter_of(w.a, data)
    s.next(B, raw=True)
    for _ in s.windows(0):
        pass
    assert "THM_SORT_RAW" in _raises(lambda: s.index(0))
    s.close()


def test_a_record_beyond_2_pow_29_is_refused():
    w = _world("test_ref")
    good = _case("no_span")
    s = _sorter_of(w.a, good + xc.make_record(1, 2 ** 31 - 2, 0, b"far", 4, [("M", 4)]))
    members, sizes, stream = _drain(s)
    assert stream == sc.sorted_stream(good + xc.make_record(1, 2 ** 31 - 2, 0, b"far", 4, [("M", 4)]), N_SQ)   # the file itself is fine
    msg = _raises(lambda: s.index(0))
    names = [n for n, _ in _sq(w)]
    assert names[1] in msg and str(2 ** 31 - 2) in msg
    assert "thm_bam_sorter_index" in _raises(lambda: s.index(0))
    s.close()
    # ending on 2^29 exactly is the last thing a .bai can address
    s = _sorter_of(w.a, xc.make_record(1, 2 ** 29 - 4, 0, b"edge", 4, [("M", 4)]))
    members, sizes, stream = _drain(s)
    _check(s, w, members, sizes, stream, N_SQ)
    s.close()


def _sq(w):
    """(name, length) of the @SQ lines of the sorted header"""
    hdr = sc.sorted_header_bytes(w.t)
    l_text, = struct.unpack_from("<I", hdr, 4)
    at, out = 12 + l_text, []
    for _ in range(struct.unpack_from("<I", hdr, 8 + l_text)[0]):
        l_name, = struct.unpack_from("<I", hdr, at)
        out.append((hdr[at + 4: at + 4 + l_name - 1].decode(), struct.unpack_from("<I", hdr, at + 4 + l_name)[0]))
        at += 8 + l_name
    return out


# ------------------------------------------------------------------ 5. the file driver
_DRIVER_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import bam_common as bc
from thermite_amd import capi
t = bc.tables("syn")
ix = capi.Index(t)
rs = bc.read_set("syn", t)
d, tag = sys.argv[1], sys.argv[2]
a = capi.Aligner(ix, rs["opts"])
try:
    st = capi.align_files(a, [d + "/reads.fastq"], "%%s/%%s.bam" %% (d, tag), capi.FMT_BAM, batch_reads=1000, n_threads=4)
    print("bytes", st["n_output_bytes"])
except capi.ThermiteError as e:
    print("error", e.code, e)
a.close()
"""


def test_file_driver_writes_the_index(tmp_path):
    w = _world("syn")
    rs = bc.read_set("syn", w.t)
    body = b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in zip(rs["names"], rs["seqs"], rs["quals"]))
    (tmp_path / "reads.fastq").write_bytes(body)
    lines = {}
    for tag, env_add in (("sorted", {"THM_BAM_SORT": "1"}), ("indexed", {"THM_BAM_SORT": "1", "THM_BAM_INDEX": "1"}), ("alone", {"THM_BAM_INDEX": "1"})):
        env = {k: v for k, v in os.environ.items() if k not in ("THM_BAM_SORT", "THM_BAM_INDEX", "THM_BAM_DEVICE", "THM_FASTQ_DEVICE")}
        env.update(env_add)
        out = subprocess.run([sys.executable, "-c", _DRIVER_CHILD % (ROOT, os.path.join(ROOT, "tests")), str(tmp_path), tag],
                             env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        lines[tag] = out.stdout.splitlines()
    bam = (tmp_path / "indexed.bam").read_bytes()
    assert bam == (tmp_path / "sorted.bam").read_bytes() and lines["indexed"] == lines["sorted"] == ["bytes %d" % len(bam)]
    assert not (tmp_path / "sorted.bam.bai").exists() and not (tmp_path / "alone.bam.bai").exists()
    assert lines["alone"][0].startswith("error %d " % capi.ERR_INVALID_ARG) and "THM_BAM_SORT" in lines["alone"][0]
    # the index against the file itself: the sorted header, the record members, the end-of-file block
    header, trailer = _header(w)
    assert bam.startswith(header) and bam.endswith(trailer) and trailer == zc.EOF_BLOCK
    off = [len(header)]
    while off[-1] < len(bam) - len(trailer):
        off.append(off[-1] + struct.unpack_from("<H", bam, off[-1] + 16)[0] + 1)
    stream = zc.check_blocks(bam[off[0]: off[-1]])[0]
    n_sq = sc.n_sq_of(w.t)
    bai = (tmp_path / "indexed.bam.bai").read_bytes()
    assert bai == xc.expected_bai(stream, n_sq, np.diff(off).tolist(), off[0])
    xc.check_queries(xc.parse_bai(bai), bam, stream, n_sq, xc.regions_of(stream, n_sq)[::4])
