"""-m gpu: run-length CIGARs and alignment summaries computed on the device (kernels_cigar.hip) against the
restatement of tests/cigar_common.py, which is built from the oracle alone: the operator-level surface
(thm_cigar_encode_batch) on hand-written and random op streams, the read level (thm_batch_fetch_cigars) against the
oracle's align_batch at both coordinate widths, both fetches of one run, the writer, and the headline batch."""
import os
import time

import numpy as np
import pytest

import cigar_common as cc
from gpu_common import MICRO_OPTS, World, assert_batch_equal, micro_exon_reads, micro_exon_reference
from oracle import aln_writer as ow
from thermite_amd import capi, refdata, synth

pytestmark = pytest.mark.gpu

TEST_OPTS = dict(min_seed_len=3, min_aln_score_percent=0.66, min_aln_score=0, multimap_score_range=1, intron_mode=False)
_worlds = {}


def _world(key, make, wide=False):
    if (key, wide) not in _worlds:
        _worlds[(key, wide)] = World(make(), wide)
    return _worlds[(key, wide)]


def _chrm(data_dir, wide=False):
    return _world("chrm", lambda: refdata.load_reference(data_dir + "/GRCh38-2020-A-chrM.fasta", data_dir + "/GRCh38-2020-A-chrM.gtf"), wide)


def _test_ref(data_dir, wide=False):
    return _world("test_ref", lambda: refdata.load_reference(data_dir + "/test_ref.fasta", data_dir + "/test_ref.gtf"), wide)


def _syn(wide=False):
    return _world("syn", lambda: synth.synth_reference(length=400000, n_genes=40), wide)


def _encode(a, streams):
    off = np.cumsum([0] + [len(s) for s in streams]).astype("<u8")
    return a.cigar_encode_batch(np.frombuffer(b"".join(streams), np.uint8), off)


def _check_streams(a, streams, what):
    r = _encode(a, streams)
    assert r.n_reads == 0 and r.offsets is None and r.alns is None and r.status is None
    dig, words = cc.expected_streams(streams)
    cc.assert_digests_equal(r.digests, r.cigar, dig, words, what)
    return r


# ------------------------------------------------------------------ operator level
M, S, D, I, X, Y = 0, 1, 2, 3, 4, 5


def hand_written_streams():
    c = cc.clip
    out = [b"", bytes([M]), bytes([S]), bytes([D]), bytes([I]), c(X, 3), c(Y, 1000), c(X, 0),
           bytes([M, S, D, I]) + c(X, 9) + c(Y, 77),                       # all six kinds
           bytes([M, S, S, M, M, S, M]),                                   # Subst / Match collapse to one M
           bytes([S, M, D, D, S, S, I, M]),
           c(Y, 40) + c(Y, 40), c(Y, 40) + c(Y, 41), c(X, 5) + c(Y, 5), c(Y, 4) + c(Y, 4) + c(Y, 4) + c(Y, 5),
           c(X, 0x04040404), c(Y, 0x05050505), c(X, 0x05040504) + c(Y, 0x04050405) + bytes([M]),   # payload bytes 04 / 05
           c(X, 4) + c(X, 5) + c(Y, 5) + c(Y, 4),
           c(X, 12) + bytes([M] * 70) + c(X, 7), c(X, 1) + c(X, 1), c(X, 2) + bytes([I, I, M, D]) + c(X, 3),   # Xclip at both ends
           c(Y, (1 << 28) - 1), c(Y, 1 << 28), bytes([M, M]) + c(Y, 0xFFFFFFFF) + bytes([M]),          # no word holds 2^28
           bytes([M]) + c(X, 1 << 28) + c(Y, 3)]
    # a clip whose five bytes start at each of the offsets 59 .. 64 of a 64-byte step (and of the second step)
    for start in range(59, 65):
        for payload in (0x00000123, 0x04050405, 0x05050505, 0x000000FF):
            for lead in (M, I):
                out.append(bytes([lead] * start) + c(Y, payload) + bytes([M, S, D]))
                out.append(bytes([lead] * (64 + start)) + c(X, payload) + c(X, payload) + bytes([I]))
                out.append(bytes([lead] * start) + c(Y, payload))                      # ... ending the stream
    # streams of exactly 63, 64, 65, 128 and 4096 bytes
    for n in (63, 64, 65, 128, 4096):
        out.append(bytes([M] * n))
        out.append(bytes([(M, S, D, I)[(k // 3) % 4] for k in range(n)]))
        out.append(bytes([M] * (n - 5)) + c(Y, 4))
        out.append(c(X, 5) + bytes([(M, D)[(k // 64) % 2] for k in range(n - 10)]) + c(X, 5))
        body = b"".join(c(Y, 5) if k % 3 else c(Y, 4) for k in range(n // 5))
        out.append(body + bytes([S] * (n - len(body))))
    for s in out:
        assert cc.well_formed(s)
    return out


def malformed_streams():
    c = cc.clip
    out = [bytes([6]), bytes([255]), bytes([M, M, 6, M]), bytes([M] * 63 + [6]), bytes([M] * 64 + [7]), c(X, 3) + bytes([9]),
           c(Y, 0x06060606) + bytes([6])]
    for kept in range(4):                      # a clip cut after 0 .. 3 payload bytes
        for lead in (0, 1, 60, 61, 62, 63, 64, 130):
            for kind in (X, Y):
                out.append(bytes([M] * lead) + c(kind, 0x04050607)[: 1 + kept])
    for s in out:
        assert not cc.well_formed(s)
    return out


@pytest.fixture(scope="module")
def enc(data_dir):
    return _test_ref(data_dir).a


def test_hand_written_streams(enc):
    good = hand_written_streams()
    r = _check_streams(enc, good, "hand-written")
    by = {s: i for i, s in enumerate(good)}

    def text(s):
        return capi.cigar_text(r.words(by[s]))

    c = cc.clip
    assert text(b"") == "*" and r.digests[by[b""]]["n_cigar"] == 0
    assert text(bytes([M, S, S, M, M, S, M])) == "7M" and text(c(Y, 40) + c(Y, 40)) == "40N" and text(c(Y, 40) + c(Y, 41)) == "40N41N"
    assert text(bytes([M, S, D, I]) + c(X, 9) + c(Y, 77)) == "2M1D1I9S77N"
    long_ = r.digests[by[c(Y, 1 << 28)]]
    assert long_["flags"] == capi.DIGEST_LONG_RUN and long_["n_cigar"] == 0 and long_["ref_len"] == 1 << 28
    assert r.digests[by[c(Y, (1 << 28) - 1)]]["flags"] == 0
    # one stream per call, and each stream between two others: neighbours do not matter
    for s in good[:40]:
        _check_streams(enc, [s], "alone")
    _check_streams(enc, good[::-1], "reversed")


def test_malformed_streams_leave_their_neighbours_alone(enc):
    good, bad = hand_written_streams(), malformed_streams()
    mixed = []
    for i, b in enumerate(bad):
        mixed += [good[(7 * i) % len(good)], b, good[(11 * i + 3) % len(good)]]
    r = _check_streams(enc, mixed, "malformed among well-formed")
    flags = r.digests["flags"].reshape(-1, 3)
    assert (flags[:, 1] == capi.DIGEST_MALFORMED).all() and not (flags[:, [0, 2]] & capi.DIGEST_MALFORMED).any()
    assert (r.digests["n_cigar"].reshape(-1, 3)[:, 1] == 0).all()
    _check_streams(enc, bad, "malformed only")


def test_encode_batch_argument_errors(enc):
    off = np.array([0, 4, 2], "<u8")
    with pytest.raises(capi.ThermiteError) as e:
        enc.cigar_encode_batch(np.zeros(4, np.uint8), off)
    assert e.value.code == capi.ERR_INVALID_ARG
    v = capi.CigarView()
    L = capi.lib()
    assert L.thm_cigar_encode_batch(enc.h, None, np.array([0, 3], "<u8").ctypes.data, 1, capi.C.byref(v)) == capi.ERR_INVALID_ARG
    assert L.thm_cigar_encode_batch(enc.h, np.zeros(4, np.uint8).ctypes.data, None, 1, capi.C.byref(v)) == capi.ERR_INVALID_ARG
    assert L.thm_cigar_encode_batch(enc.h, np.zeros(4, np.uint8).ctypes.data, off.ctypes.data, 1, None) == capi.ERR_INVALID_ARG
    r = enc.cigar_encode_batch(np.zeros(0, np.uint8), np.zeros(1, "<u8"))   # no streams
    assert len(r.digests) == 0 and len(r.cigar) == 0
    r = enc.cigar_encode_batch(np.zeros(7, np.uint8), np.array([3, 3, 7], "<u8"))   # offsets need not start at 0
    assert r.digests["n_cigar"].tolist() == [0, 1] and r.cigar.tolist() == [4 << 4]


def test_fuzz_random_streams(enc):
    """24 000 random streams, fixed seed: lengths 0 - 2000, clip density from none to heavy, clip payloads of all byte
    values, 1 % malformed, some with clips no word can hold"""
    import random
    rng = random.Random(0xC16A5)
    streams = []
    dens = [0.0, 0.002, 0.02, 0.1, 0.3, 0.6, 0.95]
    for i in range(24000):
        streams.append(cc.random_stream(rng, rng.randrange(2001), dens[i % len(dens)], malformed=rng.random() < 0.01,
                                        long_clips=rng.random() < 0.02))
    assert max(len(s) for s in streams) >= 1990 and min(len(s) for s in streams) == 0
    payload = np.zeros(256, bool)
    for s in streams[3::7][:2000]:
        payload[np.frombuffer(s, np.uint8)] = True
    assert payload.all()
    r = _check_streams(enc, streams, "fuzz")
    n_bad = int((r.digests["flags"] & capi.DIGEST_MALFORMED != 0).sum())
    assert 120 <= n_bad <= 400 and (r.digests["flags"] == capi.DIGEST_LONG_RUN).sum() > 50 and (r.digests["flags"] == 0).sum() > 20000


# ------------------------------------------------------------------ read level
def _check_read_level(w, bases, off, opts, what, n_threads=8):
    ref = w.oix.align_batch(bases, off, opts, n_threads=n_threads)
    a = w.aligner(opts)
    g = a.align_batch_cigars(bases, off)
    assert g.n_failed == 0 and g.status is None
    assert np.array_equal(g.offsets, ref.offsets), what
    for f in capi.ALN_DT.names:   # records as assert_batch_equal compares them
        if f != "pad_":
            assert np.array_equal(g.alns[f], ref.alns[f]), (what, f)
    dig, words = cc.expected_alignments(ref.alns, ref.ops)
    cc.assert_digests_equal(g.digests, g.cigar, dig, words, what)
    assert_batch_equal(a.fetch(), ref)   # the plain fetch of the same run, afterwards
    a.close()
    return g, ref


@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
def test_read_level_matches_the_oracle(data_dir, wide):
    w = _test_ref(data_dir, wide)
    _, seqs, _ = refdata.parse_fastq(data_dir + "/test_query.fastq")
    bases, off = refdata.pack_reads(seqs)
    g, _ = _check_read_level(w, bases, off, TEST_OPTS, "test_ref", n_threads=1)
    assert len(g.alns) > 0
    w = _chrm(data_dir, wide)
    bases, off, _ = synth.simulate_reads(w.t, 6000, 91, sub_rate=0.02, indel_rate=0.004, stream=31, intronic_frac=0.25)
    _check_read_level(w, bases, off, capi.CI_OPTS, "chrM")
    w = _syn(wide)
    bases, off, _ = synth.simulate_reads(w.t, 6000, 91, sub_rate=0.02, indel_rate=0.004, stream=32, intronic_frac=0.25)
    g, _ = _check_read_level(w, bases, off, capi.CI_OPTS, "spliced")
    assert ((g.cigar & 15) == 3).sum() > 500    # introns
    w = _world("micro", lambda: micro_exon_reference(), wide)
    bases, off, planned = micro_exon_reads(w.t, lengths=(91, 250), stride=13)
    g, _ = _check_read_level(w, bases, off, MICRO_OPTS, "micro-exons")
    assert int(g.digests["n_cigar"].max()) > 200   # hundreds of N words in one alignment


@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
def test_over_long_read_status(data_dir, wide):
    w = _chrm(data_dir, wide)
    sb, so, _ = synth.simulate_reads(w.t, 200, 91, stream=101)
    reads = [sb[so[i]: so[i + 1]] for i in range(200)]
    reads.insert(77, np.frombuffer(b"ACGT" * 17000, np.uint8))  # 68 000 bases
    b2, o2 = refdata.pack_reads(reads)
    a = w.aligner(capi.CI_OPTS)
    a.upload(b2, o2)
    a.run()
    f = a.fetch()
    g = a.fetch_cigars()
    assert f.n_failed == g.n_failed == 1 and np.array_equal(f.status, g.status) and g.status[77] == capi.ERR_UNSUPPORTED
    assert np.array_equal(f.offsets, g.offsets) and np.array_equal(f.alns, g.alns)
    dig, words = cc.expected_alignments(f.alns, f.ops)
    cc.assert_digests_equal(g.digests, g.cigar, dig, words, "batch with an over-long read")
    a.close()


def test_both_fetches_of_one_run(data_dir):
    w = _syn()
    bases, off, _ = synth.simulate_reads(w.t, 6000, 91, sub_rate=0.02, indel_rate=0.004, intronic_frac=0.25, stream=77)
    ref = w.oix.align_batch(bases, off, capi.CI_OPTS, n_threads=8)
    dig, words = cc.expected_alignments(ref.alns, ref.ops)
    a = w.aligner(capi.CI_OPTS)
    a.reset_counters()
    a.upload(bases, off)
    # plain fetch first: its view (not a copy) must survive the CIGAR fetches that follow
    a.run()
    view = a.fetch(copy=False)
    kept = (view.offsets.copy(), view.alns.copy(), view.ops.copy())
    t_run = a.timings()
    c_run = a.counters()
    for _ in range(3):
        g = a.fetch_cigars(copy=False)
        assert np.array_equal(g.alns, kept[1]) and np.array_equal(g.offsets, kept[0])
        cc.assert_digests_equal(g.digests, g.cigar, dig, words, "fetch, then fetch_cigars")
    assert np.array_equal(view.offsets, kept[0]) and np.array_equal(view.alns, kept[1]) and np.array_equal(view.ops, kept[2])
    assert_batch_equal(view, ref)
    t2 = a.timings()
    assert all(t2[k] == t_run[k] for k in ("seed", "plan", "extend", "compact", "total")) and t2["cigar"] > 0
    assert np.array_equal(a.counters(), c_run)
    # the other order, on a new run of the same batch; a CIGAR view stays valid over the next CIGAR fetch
    a.run()
    g1 = a.fetch_cigars(copy=False)
    k1 = (g1.digests.copy(), g1.cigar.copy(), g1.alns.copy())
    f = a.fetch()
    g2 = a.fetch_cigars(copy=False)
    assert_batch_equal(f, ref)
    assert np.array_equal(g1.digests, k1[0]) and np.array_equal(g1.cigar, k1[1]) and np.array_equal(g1.alns, k1[2])
    cc.assert_digests_equal(g2.digests, g2.cigar, dig, words, "fetch_cigars, fetch, fetch_cigars")
    assert np.array_equal(g2.alns, f.alns)
    a.close()
    # pools so small that the run overflows, grows and replays inside the CIGAR fetch
    a = w.aligner(capi.CI_OPTS)
    before = a.debug_set_pool_caps(smem_cap=300, cand_cap=16, ops_cap=4096)
    a.upload(bases, off)
    a.run()
    g = a.fetch_cigars()
    assert a.debug_set_pool_caps() > before, "the small pools did not overflow"
    assert np.array_equal(g.offsets, ref.offsets) and np.array_equal(g.alns["score"], ref.alns["score"])
    cc.assert_digests_equal(g.digests, g.cigar, dig, words, "after a pool-overflow replay")
    assert_batch_equal(a.fetch(), ref)
    a.close()


# ------------------------------------------------------------------ writer
def _fastq_batch(names, seqs, quals):
    return dict(bases=np.frombuffer(b"".join(seqs), np.uint8), offsets=np.cumsum([0] + [len(s) for s in seqs]).astype("<u8"),
                quals=np.frombuffer(b"".join(quals), np.uint8), names=np.frombuffer(b"".join(names), np.uint8),
                name_off=np.cumsum([0] + [len(n) for n in names]).astype("<u8"))


def _check_writer(ix, batch, full, cig, goldens=None):
    for fmt, key in ((capi.FMT_SAM, "sam"), (capi.FMT_PAF, "paf"), (capi.FMT_BAM, "bam")):
        for threads in (1, 4):
            wr = capi.Writer(ix, fmt, n_threads=threads)
            want = wr.format_batch(batch, full)
            got = wr.format_batch_cigars(batch, cig)
            assert got == want, (key, threads)
            if key == "bam":
                assert ow.bgzf_decompress(got + wr.trailer()) == ow.bgzf_decompress(want + wr.trailer())
            elif goldens:
                assert wr.header() + got == open(goldens[key], "rb").read(), key
            assert len(got) > 0
            wr.close()


def test_writer_from_cigars_equals_writer_from_ops(data_dir, golden_dir):
    ix = capi.Index.from_files(data_dir + "/test_ref.fasta", data_dir + "/test_ref.gtf")
    a = capi.Aligner(ix, dict(capi.DEFAULT_OPTS, min_seed_len=3, min_aln_score=0))
    rd = capi.FastqReader(data_dir + "/test_query.fastq")
    batch = rd.next_batch(1000)
    a.upload(batch["bases"], batch["offsets"])
    a.run()
    full, cig = a.fetch(), a.fetch_cigars()
    _check_writer(ix, batch, full, cig, goldens=dict(sam=os.path.join(golden_dir, "test_query.sam"), paf=os.path.join(golden_dir, "test_query.paf")))
    a.close()
    # 20 000 synthetic reads: spliced, multi-mapped (planted repeats) and unmapped (random) ones
    w = _syn()
    n = 20000
    bases, off, _ = synth.simulate_reads(w.t, n, 91, sub_rate=0.02, indel_rate=0.004, stream=41, intronic_frac=0.2)
    rng = np.random.default_rng(41)
    seqs = [bytes(bases[int(off[i]): int(off[i + 1])]) for i in range(n)]
    for i in range(0, n, 9):
        seqs[i] = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 91)])
    quals = [bytes(rng.integers(33, 74, len(s)).astype(np.uint8)) for s in seqs]
    names = [("r%d 1:N:0" % i).encode() for i in range(n)]
    batch = _fastq_batch(names, seqs, quals)
    a = w.aligner(capi.CI_OPTS)
    a.upload(batch["bases"], batch["offsets"])
    a.run()
    full, cig = a.fetch(), a.fetch_cigars()
    n_alns = np.diff(full.offsets.astype(np.int64))
    assert (n_alns == 0).sum() > 1000 and (n_alns > 1).sum() > 50
    _check_writer(w.ix, batch, full, cig)
    a.close()


# ------------------------------------------------------------------ headline batch
def test_headline_batch(capsys):
    """500 000 reads of 91 bp against the chr21-sized synthetic reference (the workload of test_gpu_fullsize.py, whose
    plain fetch is pinned to the oracle there): digests and words of every alignment against the restatement run on
    the op bytes of the plain fetch of the same run, and fewer CIGAR words than op bytes"""
    t = synth.synth_reference()
    ix = capi.Index(t, sa=capi.build_suffix_array(t["text"]))
    n = 500000
    bases, off, _ = synth.simulate_reads(t, n, 91, sub_rate=0.01, indel_rate=0.001, stream=100)
    a = capi.Aligner(ix, capi.CI_OPTS)
    a.upload(bases, off)
    a.run()
    t0 = time.perf_counter()
    f = a.fetch(copy=False)
    t1 = time.perf_counter()
    g = a.fetch_cigars(copy=False)
    t2 = time.perf_counter()
    assert np.array_equal(f.offsets, g.offsets) and np.array_equal(f.alns, g.alns)
    dig, words = cc.expected_alignments(f.alns, f.ops)
    t3 = time.perf_counter()
    cc.assert_digests_equal(g.digests, g.cigar, dig, words, "headline batch")
    assert len(g.cigar) < len(f.ops)
    with capsys.disabled():
        print("\nheadline batch: %d alignments, %d op bytes, %d CIGAR words; fetch %.1f ms (%d bytes), fetch_cigars %.1f ms (%d bytes), "
              "cigar passes %.3f ms; restatement %.1f s" % (len(f.alns), len(f.ops), len(g.cigar), (t1 - t0) * 1e3,
              f.offsets.nbytes + f.alns.nbytes + f.ops.nbytes, (t2 - t1) * 1e3, g.nbytes, a.timings()["cigar"], t3 - t2))
    a.close()
