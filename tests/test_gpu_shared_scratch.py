"""-m gpu: the scratch of the exclusive scans that the stages behind the pipeline share (thm_aligner::stage_scan_tmp,
aligner_internal.h: the CIGAR, BAM, BGZF and FASTQ passes scan through it one after the other).  One aligner takes a
small batch, a batch whose scans outgrow the scratch the small one left, and the small batch again, which then runs on
a scratch larger than it needs; every result equals what a fresh aligner gives for that batch alone, and the small
batch's also equal the oracle's.

The sizes: a first scan of at most 2048 entries asks for 80 bytes, which the buffer's growth rule makes 356 -- room for
the offsets of 36 tiles of SCAN_TILE = 2048 entries, so the scratch first grows beyond 73 728 scanned entries.  Every
read gives at least one BAM record, so 80 000 reads cross that in the BAM passes (and in the CIGAR passes, two streams
an alignment)."""
import numpy as np
import pytest

import bam_common as bc
import bgzf_common as zc
import cigar_common as cc
from fastq_device_common import batches_differ, fastq_text
from gpu_common import World
from thermite_amd import capi, synth

pytestmark = pytest.mark.gpu

N_SMALL, N_LARGE = 8, 80000
SCAN_TILE, FIRST_SCRATCH_TILES = 2048, 36


def _read_set(t, n, length, stream, tag):
    bases, off, _ = synth.simulate_reads(t, n, length, stream=stream)
    seqs = [bytes(bases[int(off[i]): int(off[i + 1])]) for i in range(n)]
    return dict(names=[b"%s%d" % (tag, i) for i in range(n)], seqs=seqs, quals=[b"I" * len(s) for s in seqs], opts=capi.CI_OPTS)


def _all_results(a, rs):
    """one run of the read set and everything the stages behind it hand out; then the same reads as a FASTQ block"""
    a.upload_reads(bc.batch_of(rs))
    a.run()
    out = dict(cig=a.fetch_cigars(), bam=a.fetch_bam(), bgzf=a.fetch_bgzf())
    info = a.upload_fastq(fastq_text(rs))
    assert info["on_device"] == 1 and info["n_reads"] == len(rs["seqs"])
    out["reads"] = a.fetch_reads()
    return out


def _assert_same(got, want, what):
    for f in ("offsets", "alns", "digests", "cigar"):
        assert np.array_equal(getattr(got["cig"], f), getattr(want["cig"], f)), (what, "fetch_cigars", f)
    for f in ("data", "read_rec_off"):
        assert np.array_equal(getattr(got["bam"], f), getattr(want["bam"], f)), (what, "fetch_bam", f)
    for f in ("data", "block_off"):
        assert np.array_equal(getattr(got["bgzf"], f), getattr(want["bgzf"], f)), (what, "fetch_bgzf", f)
    assert batches_differ(got["reads"], want["reads"]) is None, (what, "upload_fastq")
    for k in ("cig", "bam", "bgzf"):
        assert got[k].n_failed == want[k].n_failed == 0, (what, k)


def test_small_large_small_on_one_aligner():
    w = World(bc.tables("chrm"))
    small = _read_set(w.t, N_SMALL, 91, 301, b"s")
    large = _read_set(w.t, N_LARGE, 40, 302, b"L")
    fresh = {}
    for name, rs in (("small", small), ("large", large)):
        a = w.aligner(capi.CI_OPTS)
        fresh[name] = _all_results(a, rs)
        a.close()
    # the large batch's scans are longer than the scratch of the small batch's holds tile offsets for
    assert fresh["small"]["bam"].n_records < SCAN_TILE
    assert fresh["large"]["bam"].n_records >= N_LARGE > FIRST_SCRATCH_TILES * SCAN_TILE
    a = w.aligner(capi.CI_OPTS)
    for step, (name, rs) in enumerate((("small", small), ("large", large), ("small", small))):
        _assert_same(_all_results(a, rs), fresh[name], "batch %d (%s) on the shared aligner" % (step, name))
    a.close()
    # the small batch against the oracle, as test_gpu_cigar.py, test_gpu_bam.py and test_gpu_bgzf.py check theirs
    b = bc.batch_of(small)
    r = w.oix.align_batch(b["bases"], b["offsets"], capi.CI_OPTS, n_threads=4)
    assert r.counters[15] == 0
    g = fresh["small"]
    assert np.array_equal(g["cig"].offsets, r.offsets)
    for f in capi.ALN_DT.names:
        if f != "pad_":
            assert np.array_equal(g["cig"].alns[f], r.alns[f]), f
    dig, words = cc.expected_alignments(r.alns, r.ops)
    cc.assert_digests_equal(g["cig"].digests, g["cig"].cigar, dig, words, "small batch")
    data, off = bc.oracle_records(w.t, small, r)
    assert g["bam"].data.tobytes() == data and np.array_equal(g["bam"].read_rec_off, off)
    raw, _, _ = zc.check_blocks(g["bgzf"].data, g["bgzf"].block_off)
    assert raw == data
    assert batches_differ(g["reads"], b) is None
    w.ix.close()
