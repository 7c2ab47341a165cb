"""-m gpu: the coordinate sort of a run's BAM records on the device (kernels_bam_sort.hip, thm_bam_sorter).  Every case
compares bytes: the windows of the sorted stream, raw or inflated, against the oracle's record stream (or synthetic
records) split, keyed and stably sorted in Python (tests/bam_sort_common.py)."""
import ctypes
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_common as bc
import bam_sort_common as sc
import bgzf_common as zc
from gpu_common import World
from oracle import aln_writer as ow
from thermite_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = sc.BLOCK_IN
_worlds, _sets = {}, {}


def _world(key, wide=False):
    if (key, wide) not in _worlds:
        _worlds[(key, wide)] = World(bc.tables(key), wide)
    return _worlds[(key, wide)]


def _set(name, wide=False):
    """(world, read set, batch dict, oracle result, oracle record bytes); the oracle's stream is computed once"""
    w = _world(bc.REF_OF[name], wide)
    if name not in _sets:
        rs = bc.read_set(name, w.t)
        b = bc.batch_of(rs)
        r = w.oix.align_batch(b["bases"], b["offsets"], rs["opts"], n_threads=8)
        assert r.counters[15] == 0
        _sets[name] = (rs, b, r, bc.oracle_records(w.t, rs, r)[0])
    return (w,) + _sets[name]


def _raw(s, window=B):
    """the rest of the sorted stream as raw windows, joined; the windows tile it"""
    out, at = [], None
    for v in s.windows(window, raw=True):
        assert v.block_off is None and v.n_bytes == v.n_raw_bytes == len(v.data)
        assert at is None or v.raw_offset == at
        at = v.raw_offset + v.n_raw_bytes
        out.append(v.data.tobytes())
    return b"".join(out)


def _sort_records(a, data, window=B, shape=None):
    """caller-made records through the hook, finish, raw windows"""
    s = capi.BamSorter(a)
    if shape:
        s.gather_shape(shape)
    s.add_records(data)
    s.finish()
    got = _raw(s, window)
    s.close()
    return got


def _subset(rs, idx):
    return dict(rs, names=[rs["names"][i] for i in idx], seqs=[rs["seqs"][i] for i in idx],
                quals=None if rs["quals"] is None else [rs["quals"][i] for i in idx])


# ------------------------------------------------------------------ 1. read sets
@pytest.mark.parametrize("name,wide", [(n, False) for n in ("test_query", "syn", "multi", "micro", "contigs")] + [("syn", True)],
                         ids=lambda v: {False: "c32", True: "c64"}.get(v, v) if isinstance(v, bool) else v)
def test_read_sets_come_out_in_coordinate_order(name, wide):
    w, rs, b, r, data = _set(name, wide)
    n_sq = sc.n_sq_of(w.t)
    recs = [bc.parse_record(x) for x in bc.split_records(data)]
    keys = sc.keys_of(bc.split_records(data), n_sq).tolist()
    if name == "test_query":
        # n_sq = 4: the unmapped rank is 4, which a bit range of log2(n_sq) = 2 bits would lose
        assert n_sq == 4 and len({x["ref_id"] for x in recs if x["ref_id"] >= 0}) >= 2
        assert {x["flag"] & 16 for x in recs if x["ref_id"] >= 0} == {0, 16}
        assert any(x["ref_id"] < 0 for x in recs) and len(set(keys)) < len(keys)
    if name == "multi":
        # reads with 2, 3, 4 and 7 places: the records of one read, adjacent in the input, part in the sorted stream; ties
        # (equal keys from different reads) come in twos and threes
        per_read = set(np.maximum(np.diff(r.offsets.astype(np.int64)), 1).tolist())
        assert {2, 3, 4, 7} <= per_read, per_read
        assert {2, 3} <= {keys.count(k) for k in set(keys)}
    a = w.aligner(rs["opts"])
    s = capi.BamSorter(a)
    a.upload_reads(b)
    a.run()
    info = s.add()
    assert (info["n_reads"], info["n_records"], info["n_bytes"]) == (len(rs["seqs"]), len(recs), len(data))
    assert (info["total_records"], info["total_bytes"], info["n_failed_reads"]) == (len(recs), len(data), 0) and info["status"] is None
    s.finish()
    want = sc.sorted_stream(data, n_sq)
    assert want != data, "the input is in coordinate order already"
    assert _raw(s) == want
    s.close()
    a.close()


# ------------------------------------------------------------------ 2. batch splits
def test_batches_give_what_one_batch_gives():
    w, rs, b, r, data = _set("syn")
    n = len(rs["seqs"])
    rng = np.random.default_rng(77)
    junk = dict(names=[b"j%d" % i for i in range(50)], seqs=[bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 80)]) for _ in range(50)],
                quals=[b"5" * 80] * 50, opts=rs["opts"])
    cuts = [0, 1, 1700, n]
    parts = [_subset(rs, range(cuts[i], cuts[i + 1])) for i in range(3)]
    parts.insert(2, junk)   # a batch of random reads only: all unmapped
    a = w.aligner(rs["opts"])
    s = capi.BamSorter(a)
    total = 0
    for p in parts:
        a.upload_reads(bc.batch_of(p))
        a.run()
        info = s.add()
        total += info["n_records"]
        assert info["total_records"] == total
        if p is junk:
            assert info["n_records"] == 50
    s.finish()
    got = _raw(s)
    s.close()
    one = dict(rs, names=sum((p["names"] for p in parts), []), seqs=sum((p["seqs"] for p in parts), []), quals=sum((p["quals"] for p in parts), []))
    r1 = w.oix.align_batch(bc.batch_of(one)["bases"], bc.batch_of(one)["offsets"], rs["opts"], n_threads=8)
    want = sc.sorted_stream(bc.oracle_records(w.t, one, r1)[0], sc.n_sq_of(w.t))
    assert got == want
    s = capi.BamSorter(a)
    a.upload_reads(bc.batch_of(one))
    a.run()
    s.add()
    s.finish()
    assert _raw(s, 3 * B) == want
    s.close()
    a.close()


# ------------------------------------------------------------------ 3. window sizes, 4. compressed members
def test_window_sizes_and_members():
    w, rs, b, r, data = _set("syn")
    want = sc.sorted_stream(data, sc.n_sq_of(w.t))
    assert len(want) > 8 * B
    a = w.aligner(rs["opts"])
    a.upload_reads(b)
    a.run()
    members = a.debug_bgzf_device(want)[0]
    wr = capi.Writer(w.ix, capi.FMT_BAM)
    for window in (B, 3 * B, 0, 2 ** 40, 2 * B + 12345):
        for raw in (True, False):
            s = capi.BamSorter(a)
            s.add()
            s.finish()
            if raw:
                assert _raw(s, window) == want, window
                s.close()
                continue
            data_z, at, n_blocks = [], 0, 0
            step = max(B, window // B * B) if window else None
            for v in s.windows(window):
                assert (v.total_records, v.total_raw_bytes, v.raw_offset) == (len(bc.split_records(data)), len(want), at)
                assert step is None or v.n_raw_bytes == min(step, len(want) - at)
                assert v.n_blocks == -(-v.n_raw_bytes // B) and len(v.block_off) == v.n_blocks + 1
                assert v.block_off[0] == 0 and v.block_off[-1] == v.n_bytes == len(v.data)
                inflated, payload, stored = zc.check_blocks(v.data, v.block_off)
                assert inflated == want[at: at + v.n_raw_bytes]
                at += v.n_raw_bytes
                n_blocks += v.n_blocks
                data_z.append(v.data.tobytes())
            assert at == len(want) and n_blocks == -(-len(want) // B)
            z = b"".join(data_z)
            assert z == members, window   # the stream cut every 0xff00 bytes, whatever the window
            assert s.next(window).n_raw_bytes == 0   # exhausted, and stays so
            s.close()
    whole = wr.header_sorted() + members + wr.trailer()
    assert gzip.decompress(whole) == sc.sorted_header_bytes(w.t) + want
    wr.close()
    a.close()


def test_a_view_survives_the_next_call():
    w, rs, b, r, data = _set("syn")
    a = w.aligner(rs["opts"])
    a.upload_reads(b)
    a.run()
    s = capi.BamSorter(a)
    s.add()
    s.finish()
    v1 = s.next(B, copy=False)
    k1 = v1.data.copy()
    v2 = s.next(B, copy=False)
    assert v1.data.ctypes.data != v2.data.ctypes.data and np.array_equal(v1.data, k1)
    s.close()
    a.close()


# ------------------------------------------------------------------ 5. the hook
@pytest.mark.parametrize("name", ["ties", "positions", "long_record"])
def test_synthetic_records(name):
    a = _world("test_ref").a
    data = sc.synthetic_cases(4)[name]
    want = sc.sorted_stream(data, 4)
    for shape in ("pieces", "records"):
        assert _sort_records(a, data, B, shape) == want, shape
    assert _sort_records(a, data, 3 * B) == want


def test_stability_beyond_one_sort_tile():
    """100 000 forty-byte records with one key: only the ordinals order them"""
    a = _world("test_ref").a
    data = b"".join(sc.make_record(2, 1234, 16, b"%03d" % (i % 1000)) for i in range(100000))
    assert len(data) == 100000 * 40
    got = _sort_records(a, data, 16 * B)
    assert got == data


def test_keys_that_differ_in_one_field():
    a = _world("test_ref").a
    for recs in ([sc.make_record(1, 10, 16, b"rev"), sc.make_record(1, 10, 0, b"fwd")],
                 [sc.make_record(1, 11, 0, b"p11"), sc.make_record(1, 10, 0, b"p10"), sc.make_record(1, -1, 0, b"pm1"), sc.make_record(1, sc.POS_MAX, 0, b"max")],
                 [sc.make_record(-1, 10, 0, b"un"), sc.make_record(3, 10, 0, b"r3"), sc.make_record(0, 10, 0, b"r0"), sc.make_record(2, 10, 0, b"r2")]):
        data = b"".join(recs)
        want = sc.sorted_stream(data, 4)
        assert want != data and _sort_records(a, data) == want
    names = [bc.parse_record(x)["qname"] for x in bc.split_records(want)]
    assert names == [b"r0", b"r2", b"r3", b"un"]


def test_an_empty_sorter():
    w = _world("test_ref")
    s = capi.BamSorter(w.a)
    s.add_records(b"")
    s.finish()
    for raw in (True, False):
        v = s.next(0, raw)
        assert (v.n_raw_bytes, v.n_bytes, v.total_records, v.total_raw_bytes) == (0, 0, 0, 0)
    s.close()
    wr = capi.Writer(w.ix, capi.FMT_BAM)
    assert gzip.decompress(wr.header_sorted() + wr.trailer()) == sc.sorted_header_bytes(w.t)
    wr.close()


def test_malformed_records_are_refused():
    a = _world("test_ref").a
    good = sc.make_record(0, 5, 0, b"ok", l_seq=4)
    s = capi.BamSorter(a)
    for bad in (good[:-1], good + b"\x01\x02\x03", good + good[:20], b"\x10\x00\x00\x00" + bytes(16), good + b"\xff\xff\xff\xff" + bytes(40),
                sc.make_record(4, 5, 0, b"ref4"), sc.make_record(-2, 5, 0, b"refm2")):
        with pytest.raises(capi.ThermiteError) as e:
            s.add_records(bad)
        assert e.value.code == capi.ERR_INVALID_ARG, bad[:8]
    s.add_records(good)   # still usable
    s.finish()
    assert _raw(s) == good
    s.close()


# ------------------------------------------------------------------ 6. flags
def test_the_annotation_flag_passes_through():
    w, rs, b, r, data = _set("multi")
    a = w.aligner(rs["opts"])
    a.upload_reads(b)
    a.run()
    s = capi.BamSorter(a)
    s.add(capi.BAM_NO_ANNOTATION_TAGS)
    s.finish()
    stripped = bc.strip_annotation(data)
    assert stripped != data
    assert _raw(s) == sc.sorted_stream(stripped, sc.n_sq_of(w.t))
    s.close()
    a.close()


# ------------------------------------------------------------------ 7. fetch order
def test_add_among_the_fetches():
    w, rs, b, r, data = _set("multi")
    a = w.aligner(rs["opts"])
    a.upload_reads(b)
    a.run()
    alone = dict(fetch=a.fetch(), cigars=a.fetch_cigars(), bam=a.fetch_bam(), bgzf=a.fetch_bgzf())
    want = sc.sorted_stream(data, sc.n_sq_of(w.t))
    for order in (("add", "fetch", "cigars", "bam", "bgzf"), ("bgzf", "add", "bam", "cigars", "add", "fetch")):
        a.run()
        a.sync()
        c_run = a.counters()
        s = capi.BamSorter(a)
        views = {}
        for what in order:
            if what == "add":
                t0 = a.timings()
                s.add()
                assert a.timings() == t0, "add changed a timing"
            else:
                views[what] = getattr(a, {"fetch": "fetch", "cigars": "fetch_cigars", "bam": "fetch_bam", "bgzf": "fetch_bgzf"}[what])(copy=False)
        f, c, g, z = views["fetch"], views["cigars"], views["bam"], views["bgzf"]
        f0, c0, g0, z0 = alone["fetch"], alone["cigars"], alone["bam"], alone["bgzf"]
        assert np.array_equal(f.offsets, f0.offsets) and np.array_equal(f.alns, f0.alns) and np.array_equal(f.ops, f0.ops), order
        assert np.array_equal(c.digests, c0.digests) and np.array_equal(c.cigar, c0.cigar), order
        assert np.array_equal(g.data, g0.data) and np.array_equal(g.read_rec_off, g0.read_rec_off), order
        assert np.array_equal(z.data, z0.data) and np.array_equal(z.block_off, z0.block_off), order
        assert np.array_equal(a.counters(), c_run)
        s.finish()
        got = _raw(s)
        if order.count("add") == 1:
            assert got == want, order
        else:   # added twice: every record twice, the copies of one add before those of the next
            assert got == sc.sorted_stream(data + data, sc.n_sq_of(w.t)), order
        s.close()
    a.close()


# ------------------------------------------------------------------ 8. failed reads
def test_failed_reads_contribute_the_unmapped_record():
    w = _world("chrm")
    sb, so, _ = synth.simulate_reads(w.t, 200, 91, stream=101)
    seqs = [bytes(sb[so[i]: so[i + 1]]) for i in range(200)]
    seqs.insert(77, b"ACGT" * 17000)  # 68 000 bases: beyond the build limit
    rs = dict(names=[b"f%d x" % i for i in range(201)], seqs=seqs, quals=[b"I" * len(s) for s in seqs], opts=capi.CI_OPTS)
    a = w.aligner(capi.CI_OPTS)
    a.upload_reads(bc.batch_of(rs))
    a.run()
    f = a.fetch()
    s = capi.BamSorter(a)
    info = s.add()
    assert info["n_failed_reads"] == f.n_failed == 1 and np.array_equal(info["status"], f.status) and info["status"][77] == capi.ERR_UNSUPPORTED
    s.finish()
    data = bc.oracle_records(w.t, rs, f)[0]
    want = sc.sorted_stream(data, sc.n_sq_of(w.t))
    got = _raw(s)
    assert got == want
    last = bc.parse_record(bc.split_records(got)[-1])
    assert last["flag"] == 4 and last["l_seq"] == 68000 and last["qname"] == b"f77"
    s.close()
    a.close()


# ------------------------------------------------------------------ 9. the cap, 10. state errors
def test_the_cap_refuses_a_batch_and_keeps_the_rest():
    w, rs1, b1, r1, data1 = _set("test_query")
    rs = dict(rs1, names=rs1["names"] * 2, seqs=rs1["seqs"] * 2, quals=rs1["quals"] * 2)   # every read twice: over half the cap
    b = bc.batch_of(rs)
    data = bc.oracle_records(w.t, rs, w.oix.align_batch(b["bases"], b["offsets"], rs["opts"], n_threads=8))[0]
    assert len(data) <= 4096 < 2 * len(data)
    a = w.aligner(rs["opts"])
    a.upload_reads(b)
    a.run()
    s = capi.BamSorter(a, max_bytes=4096)
    s.add()
    with pytest.raises(capi.ThermiteError) as e:
        s.add()
    assert e.value.code == capi.ERR_OOM and str(2 * len(data)) in str(e.value) and "4096" in str(e.value)
    s.finish()
    assert _raw(s) == sc.sorted_stream(data, 4)
    s.close()
    a.close()


def test_state_errors():
    w, rs, b, r, data = _set("test_query")
    a = w.aligner(rs["opts"])
    s = capi.BamSorter(a)
    a.upload(b["bases"], b["offsets"])   # plain upload: no names
    a.run()
    out = []
    for call in (a.fetch_bam, s.add):
        with pytest.raises(capi.ThermiteError) as e:
            call()
        out.append((e.value.code, str(e.value)))
    assert out[0] == out[1] and out[0][0] == capi.ERR_INVALID_ARG and "thm_batch_upload_reads" in out[0][1]
    a.upload_reads(b)
    a.run()
    with pytest.raises(capi.ThermiteError) as e:
        s.add(flags=2)
    assert e.value.code == capi.ERR_INVALID_ARG and "flag" in str(e.value)
    s.add()
    with pytest.raises(capi.ThermiteError) as e:
        s.next()
    assert e.value.code == capi.ERR_INVALID_ARG and "finish" in str(e.value)
    s.finish()
    with pytest.raises(capi.ThermiteError) as e:
        s.add()
    assert e.value.code == capi.ERR_INVALID_ARG and "finish" in str(e.value)
    with pytest.raises(capi.ThermiteError) as e:
        s.add_records(sc.make_record(0, 1, 0))
    assert e.value.code == capi.ERR_INVALID_ARG
    v = capi.BamSortedView()
    assert capi.lib().thm_bam_sorter_next(s.h, 0, 2, ctypes.byref(v)) == capi.ERR_INVALID_ARG   # unknown flag bit
    assert _raw(s) == sc.sorted_stream(data, 4)
    s.close()
    a.close()


# ------------------------------------------------------------------ 11. the gather knob
def test_both_gathers_give_the_same_bytes():
    w, rs, b, r, data = _set("syn")
    want = sc.sorted_stream(data, sc.n_sq_of(w.t))
    a = w.aligner(rs["opts"])
    a.upload_reads(b)
    a.run()
    z = {}
    for shape in ("pieces", "records"):
        for window in (B, 5 * B):
            s = capi.BamSorter(a)
            assert s.gather_shape(shape) == "records" and s.gather_shape() == shape
            s.add()
            s.finish()
            assert _raw(s, window) == want, (shape, window)
            s.close()
        s = capi.BamSorter(a)
        s.gather_shape(shape)
        s.add()
        s.finish()
        z[shape] = b"".join(v.data.tobytes() for v in s.windows(2 * B))
        s.close()
    assert z["pieces"] == z["records"]
    a.close()


# ------------------------------------------------------------------ 12. the file driver
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
st = capi.align_files(a, [d + "/reads.fastq"], "%%s/%%s.bam" %% (d, tag), capi.FMT_BAM, batch_reads=1000, n_threads=4)
print("stats", st["n_reads"], st["n_aligned_reads"], st["n_records"], st["n_batches"])
print("bytes", st["n_output_bytes"])
st = capi.align_files(a, [d + "/reads.fastq"], "%%s/%%s.paf" %% (d, tag), capi.FMT_PAF, batch_reads=1000, n_threads=4)
a2 = capi.Aligner(ix, rs["opts"])
try:
    capi.align_files([a, a2], [d + "/reads.fastq"], "%%s/%%s.two.bam" %% (d, tag), capi.FMT_BAM, batch_reads=1000, n_threads=4)
    print("two ok")
except capi.ThermiteError as e:
    print("two", e.code, e)
a2.close()
a.close()
"""


def test_file_driver_writes_a_sorted_bam(tmp_path):
    """align_files with THM_BAM_SORT=1 in a child process (the switch is read from the environment): the file, inflated, is
    the oracle's header with the @HD line and the oracle's records sorted; THM_FASTQ_DEVICE=1 changes nothing; two
    aligners are refused; PAF output ignores the switch"""
    w, rs, b, r, data = _set("syn")
    body = b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in zip(rs["names"], rs["seqs"], rs["quals"]))
    (tmp_path / "reads.fastq").write_bytes(body)
    lines = {}
    for tag, env_add in (("plain", {}), ("sorted", {"THM_BAM_SORT": "1"}), ("sorted_fq", {"THM_BAM_SORT": "1", "THM_FASTQ_DEVICE": "1"})):
        env = {k: v for k, v in os.environ.items() if k not in ("THM_BAM_SORT", "THM_BAM_DEVICE", "THM_FASTQ_DEVICE")}
        env.update(env_add)
        out = subprocess.run([sys.executable, "-c", _DRIVER_CHILD % (ROOT, os.path.join(ROOT, "tests")), str(tmp_path), tag],
                             env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        lines[tag] = out.stdout.splitlines()
    want = sc.sorted_header_bytes(w.t) + sc.sorted_stream(data, sc.n_sq_of(w.t))
    plain = (tmp_path / "plain.bam").read_bytes()
    assert gzip.decompress(plain) == ow.bam_header_bytes(w.t) + data   # the unset run: the plain header, input order
    assert lines["plain"][2] == "two ok"
    for tag in ("sorted", "sorted_fq"):
        f = (tmp_path / (tag + ".bam")).read_bytes()
        assert gzip.decompress(f) == want, tag
        assert f.endswith(zc.EOF_BLOCK) and len(zc.EOF_BLOCK) == 28
        assert lines[tag][0] == lines["plain"][0], "statistics"
        assert lines[tag][1] == "bytes %d" % len(f)
        raw, payload, stored = zc.check_blocks(f, full=False)
        assert raw == want
        assert lines[tag][2].startswith("two %d " % capi.ERR_INVALID_ARG) and "THM_BAM_SORT" in lines[tag][2]
        assert (tmp_path / (tag + ".paf")).read_bytes() == (tmp_path / "plain.paf").read_bytes()
    assert len((tmp_path / "plain.paf").read_bytes()) > 100000
