"""-m gpu: BGZF members deflated on the device (kernels_bgzf.hip, thm_batch_fetch_bgzf).  Every member goes through
bgzf_common.check_blocks (header, BSIZE, a raw DEFLATE stream that Python's zlib consumes exactly, CRC-32, ISIZE); the
inflated stream is compared with thm_batch_fetch_bam of the same run, the compressed size with zlib level 1."""
import gzip
import hashlib
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import bam_common as bc
import bgzf_common as zc
from gpu_common import World
from thermite_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_worlds, _sets = {}, {}
_CASES = zc.edge_cases()


def _world(key, wide=False):
    if (key, wide) not in _worlds:
        _worlds[(key, wide)] = World(bc.tables(key), wide)
    return _worlds[(key, wide)]


def _set(name, wide=False):
    """(world, read set, batch dict)"""
    w = _world(bc.REF_OF[name], wide)
    if name not in _sets:
        rs = bc.read_set(name, w.t)
        _sets[name] = (rs, bc.batch_of(rs))
    return (w,) + _sets[name]


def _inflated(z):
    """a BgzfResult through check_blocks -> the inflated stream"""
    assert len(z.block_off) == z.n_blocks + 1
    raw, payload, stored = zc.check_blocks(z.data, z.block_off)
    assert len(raw) == z.n_raw_bytes and z.n_blocks == -(-z.n_raw_bytes // zc.BLOCK_IN)
    return raw


# ------------------------------------------------------------------ 1. the encoder alone
@pytest.mark.parametrize("name", list(_CASES))
def test_encoder_edge_cases(name):
    """len_N: the lengths around nothing, the 4 bytes a hash takes, and one, two and more than three blocks;
    zeros: 258-long matches at distance 1 and a literal alphabet of one symbol; one_byte_x7; all_256_once and
    de_bruijn_4_4: no match, so no distance code is used (the first is too short to pay for a dynamic header, the second
    keeps it); random: every block stored; motif_200: one motif repeated; twice_32768 / twice_32769: the window limit
    (a distance of 32768 is legal, 32769 is not); period_1019: every repeat straddles a 1020-byte segment boundary;
    fibonacci: byte k in proportion to Fibonacci(k), a code that needs the 15-bit limit."""
    raw = _CASES[name]
    a = _world("test_ref").a
    data, nb = a.debug_bgzf_device(raw)
    got, payload, stored = zc.check_blocks(data)
    assert got == raw and nb == len(payload) == -(-len(raw) // zc.BLOCK_IN)
    sizes = [min(zc.BLOCK_IN, len(raw) - at) for at in range(0, len(raw), zc.BLOCK_IN)]
    assert all(p <= n + 5 for p, n in zip(payload, sizes)), "a member longer than its input + 5 + 26"
    print(name, "input", len(raw), "payload", sum(payload), "stored", sum(stored), "zlib-1", zc.zlib1_payload(raw))
    if name == "random":
        assert all(stored)
    if name == "zeros":   # 253 matches of 258 and a few more tokens, a few bits each, behind a header of some tens of bytes
        assert payload[0] < 256 and not stored[0]
    if name in ("motif_200", "period_1019"):   # the first period as literals, the rest as matches
        assert sum(payload) < 2 * 1100 + len(raw) // 40 and not any(stored)
    if name == "de_bruijn_4_4":
        assert not stored[0] and payload[0] < 120   # 259 literals of two bits, and the header
    if name == "twice_32768":
        assert payload[0] < 32768 * 21 // 20 + 1024
    if name == "twice_32769":
        assert all(stored)
    if name == "fibonacci":
        assert not stored[0]
    assert a.debug_bgzf_device(raw)[0] == data, "the same bytes compress differently the second time"


# ------------------------------------------------------------------ 2. record streams
@pytest.mark.parametrize("name,wide", [(n, False) for n in ("test_query", "syn", "micro", "multi", "beyond", "contigs")] + [("syn", True)],
                         ids=lambda v: {False: "c32", True: "c64"}.get(v, v) if isinstance(v, bool) else v)
def test_members_inflate_to_the_bam_records(name, wide, tmp_path):
    w, rs, b = _set(name, wide)
    a = w.aligner(rs["opts"])
    wr = capi.Writer(w.ix, capi.FMT_BAM)
    for flags in (0, capi.BAM_NO_ANNOTATION_TAGS):
        a.upload_reads(b)
        a.run()
        a.sync()
        g = a.fetch_bam(flags)
        t0 = a.timings()
        z = a.fetch_bgzf(flags)
        t1 = a.timings()
        assert t1["bgzf"] > 0 and all(t1[k] == t0[k] for k in t0 if k != "bgzf"), (t0, t1)
        raw = _inflated(z)
        assert raw == g.data.tobytes(), (name, flags)
        assert (z.n_raw_bytes, z.n_records, z.n_reads, z.n_failed) == (len(g.data), g.n_records, g.n_reads, g.n_failed)
        assert z.status is None and z.n_failed == 0
        z2 = a.align_batch_bgzf(b, flags)   # upload + run + fetch
        assert np.array_equal(z2.data, z.data) and np.array_equal(z2.block_off, z.block_off) and z2.n_records == z.n_records
        # header + members + trailer is a .bam file: Python's gzip and the library's own inflater, serial and parallel
        whole = wr.header() + z.data.tobytes() + wr.trailer()
        want = gzip.decompress(wr.header()) + raw
        assert gzip.decompress(whole) == want
        path = tmp_path / ("%d.bam" % flags)
        path.write_bytes(whole)
        for threads in (1, 4):
            assert capi.debug_gunzip(path, threads=threads) == want, threads
    wr.close()
    a.close()


# ------------------------------------------------------------------ 3. determinism
def test_the_same_records_give_the_same_bytes():
    w, rs, b = _set("syn")
    a = w.aligner(rs["opts"])
    z1 = a.align_batch_bgzf(b)
    z2 = a.align_batch_bgzf(b)
    a2 = w.aligner(rs["opts"])
    z3 = a2.align_batch_bgzf(b)
    assert z1.n_blocks >= 8
    assert np.array_equal(z1.data, z2.data) and np.array_equal(z1.data, z3.data)
    assert np.array_equal(z1.block_off, z3.block_off)
    a.close()
    a2.close()


# ------------------------------------------------------------------ 4. compression
@pytest.mark.parametrize("name", ["syn", "chrm_ci", "multi"])
def test_no_larger_than_zlib_level_1(name):
    """total payload bytes (members without the 26 bytes of header and tail) against zlib level 1 over the same cuts:
    device <= zlib-1, no margin.  The host encoder's total for the same records is printed beside them.
    (syn and chrm_ci are 16 and 11 blocks; multi is a single block of 52 KB.)"""
    w, rs, b = _set(name)
    a = w.aligner(rs["opts"])
    a.upload_reads(b)
    a.run()
    g = a.fetch_bam()
    z = a.fetch_bgzf()
    raw, payload, stored = zc.check_blocks(z.data, z.block_off)
    assert raw == g.data.tobytes()
    wr = capi.Writer(w.ix, capi.FMT_BAM, n_threads=1)
    host = sum(zc.check_blocks(wr.wrap_bam(g), full=False)[1])
    wr.close()
    a.close()
    ref = zc.zlib1_payload(raw)
    print("%s: %d bytes in %d blocks; payload device %d, host encoder %d, zlib level 1 %d" % (name, len(raw), len(payload), sum(payload), host, ref))
    assert sum(payload) <= ref


# ------------------------------------------------------------------ 5. fetch order
def test_the_four_fetches_in_every_order():
    w, rs, b = _set("multi")
    a = w.aligner(rs["opts"])
    a.upload_reads(b)
    first = None
    for order in itertools.permutations(("fetch", "cigars", "bam", "bgzf")):
        a.run()
        a.sync()
        c_run = a.counters()
        views, kept = {}, {}
        for what in order:
            if what == "fetch":
                v = a.fetch(copy=False)
                kept[what] = (v.offsets.copy(), v.alns.copy(), v.ops.copy())
            elif what == "cigars":
                v = a.fetch_cigars(copy=False)
                kept[what] = (v.offsets.copy(), v.alns.copy(), v.digests.copy(), v.cigar.copy())
            elif what == "bam":
                v = a.fetch_bam(copy=False)
                kept[what] = (v.read_rec_off.copy(), v.data.copy())
            else:
                v = a.fetch_bgzf(copy=False)
                kept[what] = (v.block_off.copy(), v.data.copy())
            views[what] = v
        f, c, g, z = views["fetch"], views["cigars"], views["bam"], views["bgzf"]
        now = {"fetch": (f.offsets, f.alns, f.ops), "cigars": (c.offsets, c.alns, c.digests, c.cigar), "bam": (g.read_rec_off, g.data),
               "bgzf": (z.block_off, z.data)}
        # every view is still valid after the other three fetches ...
        assert all(np.array_equal(x, y) for k in now for x, y in zip(now[k], kept[k])), order
        # ... and what it is alone (the first order's copies), whatever the order
        if first is None:
            first = kept
        assert all(np.array_equal(x, y) for k in kept for x, y in zip(kept[k], first[k])), order
        assert _inflated(z) == g.data.tobytes()
        assert np.array_equal(a.counters(), c_run)
    # the two-set rule: a BGZF view survives the next BGZF fetch
    a.run()
    z1 = a.fetch_bgzf(copy=False)
    k1 = z1.data.copy()
    a.run()
    z2 = a.fetch_bgzf(copy=False)
    assert z1.data.ctypes.data != z2.data.ctypes.data
    assert np.array_equal(z1.data, k1) and np.array_equal(z2.data, k1)
    a.close()


# ------------------------------------------------------------------ 6. further cases
def test_empty_batch_and_a_batch_without_alignments():
    w = _world("syn")
    a = w.aligner(capi.CI_OPTS)
    empty = dict(bases=np.zeros(0, np.uint8), offsets=np.zeros(1, "<u8"), quals=None, names=np.zeros(0, np.uint8), name_off=np.zeros(1, "<u8"))
    z = a.align_batch_bgzf(empty)
    assert (z.n_reads, z.n_records, z.n_blocks, z.n_raw_bytes, len(z.data)) == (0, 0, 0, 0, 0) and z.block_off.tolist() == [0]
    rng = np.random.default_rng(5)
    seqs = [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 60 + i % 5)]) for i in range(300)]
    rs = dict(names=[b"n%d" % i for i in range(300)], seqs=seqs, quals=[b"#" * len(s) for s in seqs], opts=capi.CI_OPTS)
    b = bc.batch_of(rs)
    z = a.align_batch_bgzf(b)
    g = a.fetch_bam()
    assert z.n_records == 300 and all(bc.parse_record(r)["flag"] == 4 for r in bc.split_records(g.data))
    assert _inflated(z) == g.data.tobytes()
    a.close()


def test_after_a_pool_overflow_replay():
    w, rs, b = _set("syn")
    a = w.aligner(rs["opts"])
    want = a.align_batch_bam(b).data.tobytes()
    before = a.debug_set_pool_caps(smem_cap=300, cand_cap=16, ops_cap=4096)
    a.upload_reads(b)
    a.run()
    z = a.fetch_bgzf()   # the replay happens inside this call's sync
    assert a.debug_set_pool_caps() > before, "the small pools did not overflow"
    assert _inflated(z) == want
    a.close()


def test_failed_reads_get_the_unmapped_record():
    w = _world("chrm")
    sb, so, _ = synth.simulate_reads(w.t, 200, 91, stream=101)
    seqs = [bytes(sb[so[i]: so[i + 1]]) for i in range(200)]
    seqs.insert(77, b"ACGT" * 17000)  # 68 000 bases: beyond the build limit
    rs = dict(names=[b"f%d x" % i for i in range(201)], seqs=seqs, quals=[b"I" * len(s) for s in seqs], opts=capi.CI_OPTS)
    a = w.aligner(capi.CI_OPTS)
    a.upload_reads(bc.batch_of(rs))
    a.run()
    g = a.fetch_bam()
    z = a.fetch_bgzf()
    assert z.n_failed == g.n_failed == 1 and np.array_equal(z.status, g.status) and z.status[77] == capi.ERR_UNSUPPORTED
    raw = _inflated(z)
    assert raw == g.data.tobytes()
    rec = bc.parse_record(raw[int(g.read_rec_off[77]): int(g.read_rec_off[78])])
    assert rec["flag"] == 4 and rec["l_seq"] == 68000 and rec["qname"] == b"f77"
    a.close()


# ------------------------------------------------------------------ 7. errors
def test_errors_are_those_of_fetch_bam():
    w, rs, b = _set("multi")
    a = w.aligner(rs["opts"])

    def both(prepare, **kw):
        out = []
        for call in (a.fetch_bam, a.fetch_bgzf):
            prepare()
            with pytest.raises(capi.ThermiteError) as e:
                call(**kw)
            out.append((e.value.code, str(e.value)))
        assert out[0] == out[1], out
        return out[1]

    def plain():
        a.upload(b["bases"], b["offsets"])   # plain upload: no names
        a.run()

    code, msg = both(plain)
    assert code == capi.ERR_INVALID_ARG and "thm_batch_upload_reads" in msg

    def named():
        a.upload_reads(b)
        a.run()

    for bad in (2, 0x80000000, 3):
        code, msg = both(named, flags=bad)
        assert code == capi.ERR_INVALID_ARG and "flag" in msg
    names = list(rs["names"])
    names[5] = b"q" * 255 + b" x"
    long_b = bc.batch_of(dict(rs, names=names))

    def long_name():
        a.upload_reads(long_b)
        a.run()

    code, msg = both(long_name)
    assert code == capi.ERR_INTERNAL and "read name longer than 254 bytes cannot be stored in BAM" in msg
    named()
    assert _inflated(a.fetch_bgzf()) == a.fetch_bam().data.tobytes()   # the next batch after the failed ones
    a.close()


# ------------------------------------------------------------------ 8. driver
_DRIVER_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import bam_common as bc
from thermite_amd import capi
t = bc.tables("syn")
ix = capi.Index(t)
rs = bc.read_set("syn", t)
for n_al in (1, 2):
    als = [capi.Aligner(ix, rs["opts"]) for _ in range(n_al)]
    st = capi.align_files(als, [sys.argv[1] + "/reads.fastq"], "%%s/%%s.%%d.bam" %% (sys.argv[1], sys.argv[2], n_al), capi.FMT_BAM, batch_reads=700, n_threads=4)
    print("stats", n_al, st["n_reads"], st["n_aligned_reads"], st["n_records"], st["n_batches"])
    print("bytes", n_al, st["n_output_bytes"])
    for a in als:
        a.close()
"""


def test_file_driver_with_the_device_compressor(tmp_path):
    """align_files(FMT_BAM) with THM_BAM_DEVICE unset, 1 and 2 (a child process per setting, one at a time; the switch
    is read from the environment), one and two aligners: the files gunzip to the same bytes, the statistics agree, the
    =2 file is device members throughout, closed by the end-of-file block, and n_output_bytes is its size"""
    w, rs, b = _set("syn")
    body = b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in zip(rs["names"], rs["seqs"], rs["quals"]))
    (tmp_path / "reads.fastq").write_bytes(body)
    stats, nbytes = {}, {}
    for tag, switch in (("host", None), ("records", "1"), ("members", "2")):
        env = dict(os.environ)
        env.pop("THM_BAM_DEVICE", None)
        if switch is not None:
            env["THM_BAM_DEVICE"] = switch
        out = subprocess.run([sys.executable, "-c", _DRIVER_CHILD % (ROOT, os.path.join(ROOT, "tests")), str(tmp_path), tag],
                             env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        stats[tag] = [ln for ln in out.stdout.splitlines() if ln.startswith("stats")]
        nbytes[tag] = [int(ln.split()[2]) for ln in out.stdout.splitlines() if ln.startswith("bytes")]
        assert len(stats[tag]) == 2
    assert stats["host"] == stats["records"] == stats["members"]   # reads, aligned reads, records, batches
    wr = capi.Writer(w.ix, capi.FMT_BAM)
    header, trailer = wr.header(), wr.trailer()
    wr.close()
    assert trailer == zc.EOF_BLOCK
    for k, n_al in enumerate((1, 2)):
        files = {tag: (tmp_path / ("%s.%d.bam" % (tag, n_al))).read_bytes() for tag in stats}
        want = gzip.decompress(files["host"])
        assert gzip.decompress(files["records"]) == want and gzip.decompress(files["members"]) == want, n_al
        m = files["members"]
        assert m.endswith(zc.EOF_BLOCK) and m.startswith(header) and nbytes["members"][k] == len(m)
        raw, payload, stored = zc.check_blocks(m, full=False)   # member by member; the header's and the end-of-file block too
        assert raw == want
        assert capi.debug_gunzip(tmp_path / ("members.%d.bam" % n_al), threads=4) == want


# ------------------------------------------------------------------ 9. C++
def test_cpp_align_reads_bgzf(data_dir, tmp_path):
    exe = tmp_path / "bgzf_main"
    libdir = os.path.dirname(capi.SO_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "bgzf_main.cpp"), "-o", str(exe), "-L" + libdir,
                           "-lthermite_amd", "-lz", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    idx = tmp_path / "test_ref.thmidx"
    ix = capi.Index.from_files(data_dir + "/test_ref.fasta", data_dir + "/test_ref.gtf")
    ix.save(idx)
    m_out = tmp_path / "members.bin"
    out = subprocess.run([str(exe), str(idx), "3", "0", data_dir + "/test_query.fastq", str(m_out)], check=True, capture_output=True, timeout=120)
    w, rs, b = _set("test_query")
    a = capi.Aligner(ix, rs["opts"])
    z = a.align_batch_bgzf(b)
    raw = _inflated(z)
    assert raw == open(bc.GOLDEN_BIN, "rb").read()
    assert m_out.read_bytes() == z.data.tobytes()
    assert out.stdout.decode().split() == ["blocks", "%d" % z.n_blocks, "records", "%d" % z.n_records, "raw", "%d" % len(raw), "sha256",
                                           hashlib.sha256(raw).hexdigest()]
    a.close()
    ix.close()
