"""-m gpu: the many-contig world of tests/contigs_common.py through every layer, byte for byte against the CPU oracle.
What only this world reaches: idx_to_ref with many contig-copy boundaries in one bin (extend_device.h, kernels_hit.hip,
kernels_tpr.hip, smem_finish.h), the three restatements of filter_overlapping with alignments that overlap on different
contigs and a name_rank that differs between them (kernels_extend.hip register and list path, kernels_tpr.hip), window
clamps on contigs shorter than a read, and -- downstream -- refIDs that are not name ranks (BAM, sorter, .bai, thm_quant,
thm_coverage).  tests/test_contigs_host.py asserts from the oracle alone that the reads do reach each of these."""
import contextlib
import gzip
import os
import struct

import numpy as np
import pytest

import bai_common as xc
import bam_common as bc
import bam_sort_common as sc
import bgzf_common as zc
import contigs_common as cg
import cov_common as cv
import gpu_common as gc
import quant_common as qc
import smem_finish_common as sf
from oracle import aln_writer as ow
from oracle import pyoracle as orc
from thermite_amd import capi, refdata

pytestmark = pytest.mark.gpu

WIDTHS = pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
KNOBS = ("THM_COVERAGE", "THM_QUANT", "THM_BAM_SORT", "THM_BAM_INDEX", "THM_BAM_DEVICE", "THM_FASTQ_DEVICE")
READ_LEVEL_OPTS = {
    "ci": capi.CI_OPTS,
    "default": capi.DEFAULT_OPTS,
    "range0": dict(capi.CI_OPTS, multimap_score_range=0),
    "range5": dict(capi.CI_OPTS, multimap_score_range=5),
    "no_introns": dict(capi.CI_OPTS, intron_mode=False),
}
_memo = {}


def _world(wide=False):
    if ("w", wide) not in _memo:
        _memo[("w", wide)] = gc.World(cg.world()[0], wide)
    return _memo[("w", wide)]


def _reads(name="general"):
    if ("reads", name) not in _memo:
        _memo[("reads", name)] = cg.pack(cg.read_set(name))
    return _memo[("reads", name)]


def _oracle(name, key, opts):
    """the oracle's result for a read set under the options called `key`, computed once and left unchanged"""
    if ("oracle", name, key) not in _memo:
        bases, off = _reads(name)
        r = _world().oix.align_batch(bases, off, opts, n_threads=8)
        assert r.counters[15] == 0
        _memo[("oracle", name, key)] = r
    return _memo[("oracle", name, key)]


def _n_alns(r):
    return np.diff(r.offsets.astype(np.int64))


# ------------------------------------------------------------------ 1. seeds
@WIDTHS
@pytest.mark.parametrize("k", [20, 12])
def test_seeds(k, wide):
    bases, off = _reads()
    gc.check_smems(_world(wide), bases, off, k)


# ------------------------------------------------------------------ 2. read level
@WIDTHS
@pytest.mark.parametrize("key", list(READ_LEVEL_OPTS))
def test_read_level(key, wide):
    bases, off = _reads()
    opts = READ_LEVEL_OPTS[key]
    r = _oracle("general", key, opts)
    gc.check_align(_world(wide), bases, off, opts, ref=r)
    if key == "ci":
        # (the floors of tests/test_contigs_host.py hold for this result; two of them again, cheaply)
        contig = cg.contig_of(cg.world()[0], r.alns["ref_id"])
        assert len(set(contig.tolist())) >= 60 and (_n_alns(r) > cg.KEYCAP).sum() >= 20


def test_read_level_with_pools_that_overflow():
    bases, off = _reads()
    gc.check_align(_world(), bases, off, capi.CI_OPTS, pool_caps=dict(smem_cap=300, cand_cap=16, ops_cap=4096), ref=_oracle("general", "ci", capi.CI_OPTS))


@WIDTHS
def test_contigs_too_short_for_the_score_threshold(wide):
    """the contigs of 1, 2, k - 1 and k bases, each inside a read, with a threshold that lets k matching bases through"""
    bases, off = _reads("tiny")
    r = _oracle("tiny", "tiny", cg.TINY_OPTS)
    t, info = cg.world()
    assert info["index_of"]["z%d" % cg.K] in set(cg.contig_of(t, r.alns["ref_id"]).tolist())
    gc.check_smems(_world(wide), bases, off, cg.K)
    gc.check_align(_world(wide), bases, off, cg.TINY_OPTS, ref=r)


# ------------------------------------------------------------------ 3. the three restatements of filter_overlapping
def _tpr_stats(w, bases, off, opts):
    a = w.aligner(opts)
    a.debug_set_flags(tpr=True)
    a.align_batch(bases, off)
    st = a.debug_tpr_stats()
    a.close()
    return st


@WIDTHS
def test_filter_list_path_of_the_wave_per_read_kernel(wide):
    """reads from the 24 exact copies: more than KEYCAP accepted candidates each, on six contigs, in the fast class"""
    w = _world(wide)
    bases, off = _reads("list")
    r = _oracle("list", "ci", capi.CI_OPTS)
    lens = np.diff(off.astype(np.int64))
    assert sf.fast_class(capi.CI_OPTS, lens)[0] == lens.max() <= cg.L0 + 4   # every read in the register-resident class
    f2 = np.array(cg.read_set("list")["kinds"]) == "F2"
    many = f2 & (_n_alns(r) > cg.KEYCAP)
    assert many.sum() >= 40
    contig = cg.contig_of(w.t, r.alns["ref_id"])
    o = r.offsets.astype(np.int64)
    assert all(len(set(contig[o[i]: o[i + 1]].tolist())) >= 3 for i in np.nonzero(many)[0])
    a = w.aligner(capi.CI_OPTS)
    hits = np.diff(a.smems_batch(bases, off, cg.K)[0].astype(np.int64))
    a.close()
    assert (hits[f2] < gc.TEAM_HITS).all()                                # ... and not the team kernel's
    gc.check_align(w, bases, off, capi.CI_OPTS, ref=r)                    # the problem-parallel path on, then off
    assert _tpr_stats(w, bases, off, capi.CI_OPTS)[16] > 0


@WIDTHS
def test_filter_in_the_any_width_kernel(wide):
    """300-base tilings of the paralogous segment, band +-150: beyond four cells per lane, so the any-width kernel aligns
    them and its list path filters what lies at one coordinate of four contigs"""
    w = _world(wide)
    bases, off = _reads("wide")
    r = _oracle("wide", "wide", cg.WIDE_OPTS)
    lens = np.diff(off.astype(np.int64))
    assert gc.initial_band(cg.WIDE_OPTS, 300) == 150 and sf.fast_class(cg.WIDE_OPTS, [300])[0] == 0
    long = lens == 300
    contig = cg.contig_of(w.t, r.alns["ref_id"])
    o = r.offsets.astype(np.int64)
    n_multi = sum(1 for i in np.nonzero(long)[0] if len(set(contig[o[i]: o[i + 1]].tolist())) >= 3)
    assert long.sum() >= 100 and n_multi >= 100, (int(long.sum()), n_multi)
    gc.check_align(w, bases, off, cg.WIDE_OPTS, ref=r)


@WIDTHS
def test_filter_in_the_team_kernel(wide):
    """reads from the diverged family: TEAM_HITS seed hits and more, over six contigs; the heavy list beside them"""
    w = _world(wide)
    bases, off = _reads("team")
    r = _oracle("team", "ci", capi.CI_OPTS)
    a = w.aligner(capi.CI_OPTS)
    hits = np.diff(a.smems_batch(bases, off, cg.K)[0].astype(np.int64))
    a.close()
    assert (hits >= gc.TEAM_HITS).sum() >= 4 and hits.max() <= gc.TEAM_MAX_HITS and ((hits >= 8) & (hits < 32)).sum() >= 4
    contig = cg.contig_of(w.t, r.alns["ref_id"])
    o = r.offsets.astype(np.int64)
    team = np.nonzero(hits >= gc.TEAM_HITS)[0]
    assert sum(1 for i in team if len(set(contig[o[i]: o[i + 1]].tolist())) >= 2) >= 4
    for key in ("ci", "range5"):
        opts = READ_LEVEL_OPTS[key]
        gc.check_align(w, bases, off, opts, ref=_oracle("team", key, opts))
    assert _tpr_stats(w, bases, off, capi.CI_OPTS)[16] > 0


# ------------------------------------------------------------------ 4. the finisher
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sf.host_program(tmp_path_factory.mktemp("contigs_finish"))


@WIDTHS
def test_finisher(exe, wide, tmp_path):
    """ref_of and the window clamps of smem_finish.h on contigs other than the first: records, op streams and counters
    against the oracle, the device's finished / left counts against the host program's"""
    w = _world(wide)
    bases, off = _reads()
    c = sf.check_device(exe, w, capi.CI_OPTS, (bases, off), tmp_path)
    out, _ = sf.run_host(exe, w, capi.CI_OPTS, bases, off, tmp_path)
    assert sf.finished_counts(out) == c
    later = cg.contig_of(w.t, out["ref_id"].clip(0, len(w.t["refs"]) - 1)) != 0
    done = (out["what"] == 1) & (out["accepted"] > 0)
    assert (done & later & (out["shape"] == 1)).sum() >= 20 and (done & later & (out["shape"] == 2)).sum() >= 20
    assert (done & later & (out["ystart"] == 0)).sum() >= 4 and (done & later & (out["yend"] == out["ylen"])).sum() >= 4


# ------------------------------------------------------------------ 5. the per-hit layer
def _per_hit_expected(w, bases, off, hit_off, hits, narrow):
    """bands, X-drops and the restatement's records for the hits; the restatement runs once per band choice"""
    key = ("per_hit", narrow)
    if key not in _memo:
        rng = np.random.default_rng(31)
        per_hit_len = np.repeat(np.diff(off.astype(np.int64)), np.diff(hit_off.astype(np.int64)))
        bw0 = np.array([gc.initial_band(capi.CI_OPTS, int(n)) for n in per_hit_len], "<u4")
        if narrow:
            bw = (bw0 * rng.random(len(bw0))).astype("<u4")
            xd = (bw + rng.integers(0, 6, len(bw))).astype("<i4")
        else:
            bw, xd = bw0, bw0.astype("<i4")
        max_bw = int(bw0.max())
        _memo[key] = (hits.copy(), bw, xd, max_bw, gc.expected_batch(w, bases, off, hit_off, hits, bw, xd, max_bw))
    first, bw, xd, max_bw, exp = _memo[key]
    assert np.array_equal(first, hits)    # (the seeds do not depend on the index's width)
    return bw, xd, max_bw, exp


@WIDTHS
def test_per_hit_entry_points(wide):
    """thm_align_seed_hits_batch on contig-end reads, reads that join two contigs and reads from the paralogs against the
    restatement of align_seed_hit; thm_extend_left_right_batch on the same hits, each with the genome window that
    align_seed_hit cuts (src/aligner.rs:206-213: clamped at the contig copy's start and at its '$')"""
    w = _world(wide)
    bases, off = _reads("per_hit")
    kinds = cg.read_set("per_hit")["kinds"]
    assert 200 <= len(kinds) <= 400 and kinds.count("end_join") >= 40 and kinds.count("end_whole") >= 20
    hit_off, hits = w.a.smems_batch(bases, off, cg.K)
    refs, text = w.t["refs"], w.t["text"]
    on = cg.contig_of(w.t, np.searchsorted(refs["end_idx"], hits["ref_idx"], side="right"))
    assert len(hits) >= 300 and len(set(on.tolist())) >= 30
    for narrow in (False, True):
        bw, xd, max_bw, exp = _per_hit_expected(w, bases, off, hit_off, hits, narrow)
        gc.assert_hits_equal(w.a.align_seed_hits(bases, off, hit_off, hits, bw, xd, max_bw), exp, "narrow" if narrow else "initial")
    # extend_left_right on the clamped windows
    bw, xd, max_bw, _ = _per_hit_expected(w, bases, off, hit_off, hits, False)
    read_of = np.repeat(np.arange(len(off) - 1), np.diff(hit_off.astype(np.int64)))
    xs, ys, local, clamped = [], [], np.zeros(len(hits), capi.MEM_DT), 0
    for h, m in enumerate(hits):
        read = bases[int(off[read_of[h]]): int(off[read_of[h] + 1])]
        hr, q, ln, L = int(m["ref_idx"]), int(m["query_idx"]), int(m["len"]), len(read)
        ref = refs[int(np.searchsorted(refs["end_idx"], hr, side="right"))]
        s0, s1 = max(hr - (L + int(bw[h])), 0, int(ref["start_idx"])), min(hr + ln + L + int(bw[h]), int(ref["end_idx"]) - 1)
        clamped += (s0 == int(ref["start_idx"])) + (s1 == int(ref["end_idx"]) - 1)
        xs.append(sf.sanitise(read))
        ys.append(text[s0:s1])
        local[h] = (hr - s0, q, ln)
    assert clamped >= 200, clamped
    xb, xo = refdata.pack_reads(xs)
    yb, yo = refdata.pack_reads(ys)
    alns, ops = w.a.extend_left_right_batch(xb, xo, yb, yo, local, bw, xd, max_bw)
    swg = orc.Swg(max_bw)
    for h in range(len(hits)):
        e = swg.extend_left_right(ys[h], tuple(int(v) for v in local[h]), xs[h], int(bw[h]), int(xd[h]))
        a = alns[h]
        got = tuple(int(a[f]) for f in ("score", "ystart", "xstart", "yend", "xend", "ylen", "xlen"))
        assert got == (e["score"], e["ystart"], e["xstart"], e["yend"], e["xend"], e["ylen"], e["xlen"]), (h, got, e)
        assert orc.decode_ops(ops[a["ops_off"]: a["ops_off"] + a["ops_len"]]) == e["ops"], h


# ------------------------------------------------------------------ 6. downstream of one run
def _sq_mismatch(t):
    """file indices (BAM refIDs) of the contigs whose name rank is another number"""
    return set(np.nonzero(t["name_rank"] != np.arange(len(t["names"])))[0].tolist())


@WIDTHS
def test_quant_tables(wide):
    w = _world(wide)
    bases, off = _reads()
    r = _oracle("general", "ci", capi.CI_OPTS)
    if "quant" not in _memo:
        _memo["quant"] = qc.from_oracle(w.t, r)
    exp = _memo["quant"]
    a = w.aligner(capi.CI_OPTS)
    q = capi.Quant(a)
    a.upload(bases, off)
    a.run()
    info = q.add()
    got = qc.of_result(q.fetch())
    qc.assert_tables_equal(got, exp)
    qc.check_invariants(got)
    assert {k: info[k] for k in qc.TOTAL_NAMES} == exp["totals"] and info["n_junctions"] == len(exp["junctions"]) >= 40
    # a junction's ref_id is the BAM refID (file order), not the name rank: rows on contigs where the two differ, and on
    # the contigs the spliced transcripts lie on only
    j = got["junctions"]
    spliced = set(cg.world()[1]["tx_contig"][w.t["txs"]["n_exons"] > 1].tolist())
    assert set(j["ref_id"].tolist()) <= spliced and len(set(j["ref_id"].tolist()) & _sq_mismatch(w.t)) >= 3
    assert np.array_equal(j["ref_id"], np.sort(j["ref_id"]))
    assert (got["genes"]["exonic_unique"][cg.world()[1]["edge_genes"]] > 0).all()
    q.close()
    a.close()


def _cov_expect(flags):
    if ("cov", flags) not in _memo:
        _memo[("cov", flags)] = cv.from_oracle(cg.world()[0], flags, _oracle("general", "ci", capi.CI_OPTS))
    return _memo[("cov", flags)]


@pytest.mark.parametrize("flags", cv.ALL_FLAGS)
def test_coverage_tracks(flags):
    w = _world()
    t, info = cg.world()
    bases, off = _reads()
    exp = _cov_expect(flags)
    n_sq = len(t["names"])
    assert cv.sq_lengths(t) == info["lens"].tolist()
    a = w.aligner(capi.CI_OPTS)
    c = capi.Coverage(a, flags)
    a.upload(bases, off)
    a.run()
    got = c.add()
    assert {k: got[k] for k in cv.TOTAL_NAMES + ["track"]} == exp.totals
    run = np.nonzero(info["kind"] == "tiny")[0]
    z1, z20 = info["index_of"]["z1"], info["index_of"]["z%d" % cg.K]
    ranges = [(0, n_sq), (int(run[0]), len(run)), (int(run[2]), 1), (int(run[-1]), 1), (z1, 1), (z1, 4), (z20, 1), (n_sq - 1, 1),
              (info["index_of"][cg.SCAF_ALL_N], 1), (info["index_of"][cg.SCAF_WHOLE_91], 2)]
    for k in range(cv.n_tracks(flags)):
        for first, n in ranges:
            cv.check_result(c.fetch(k, first, n), exp, k, first, n, "track %d refs [%d, +%d)" % (k, first, n))
        # windows of depths that end on a contig's last base: a large contig with a gene flush with its end, a contig of one
        # read's length, a tiny one
        for ci in (info["index_of"]["chr2"], info["index_of"]["chr10"], info["index_of"][cg.SCAF_WHOLE_91], int(run[0])):
            n = int(info["lens"][ci])
            m = min(n, 700)
            assert np.array_equal(c.depth(k, ci, n - m, m), exp.depth(k, ci)[n - m:]), (k, ci)
    if flags == cv.MULTI:
        d = exp.depth(0, info["index_of"]["chr2"])
        assert d[-100:].min() > 0 and d[:100].min() > 0     # the edge genes are covered to the contig's first and last base
        assert sum(1 for ci in run if exp.depth(0, int(ci)).any()) >= 10
    c.close()
    a.close()


# ------------------------------------------------------------------ 7. the file driver
@contextlib.contextmanager
def _knobs(**kv):
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def test_file_driver(tmp_path):
    """FASTQ of the general read set -> SAM as the oracle renders it (one aligner, two on the one device); with the sorted
    BAM, its index, the count tables and the coverage tracks asked for together, each is what its own layer's test expects"""
    w = _world()
    t = w.t
    rs = bc.read_set("contigs", t)
    r = _oracle("general", "ci", capi.CI_OPTS)
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in zip(rs["names"], rs["seqs"], rs["quals"])))
    a, a2 = w.aligner(capi.CI_OPTS), w.aligner(capi.CI_OPTS)
    want_sam = ow.sam_header(t) + ow.format_batch(t, rs["names"], rs["seqs"], rs["quals"], r, "sam")
    for tag, aligners in (("one", a), ("two", [a, a2])):
        with _knobs():
            capi.align_files(aligners, [fq], tmp_path / tag, capi.FMT_SAM, batch_reads=700, n_threads=4)
        assert (tmp_path / tag).read_bytes() == want_sam, tag
    # the run's own SAM, counted line by line, says what the oracle's alignments say
    sam = str(tmp_path / "one")
    exp_q = qc.from_oracle(t, r)
    want_tables = qc.tsv_of(t, exp_q)
    genes, rows = qc.count_sam(sam, t)
    assert qc.tsv_of_sam_counts(t, genes, rows) == want_tables
    sq, n_sq = qc.sq_names(t), len(t["names"])
    for flags in cv.ALL_FLAGS:
        exp_c = _cov_expect(flags)
        depth = cv.sam_depth(sam, t, flags)
        tracks = {name: cv.bedgraph(sq, depth[k]) for k, name in enumerate(cv.track_names(flags))}
        assert tracks == {name: cv.bedgraph(sq, [exp_c.depth(k, s) for s in range(n_sq)]) for k, name in enumerate(cv.track_names(flags))}, flags
        if flags == cv.STRANDED | cv.MULTI:
            want_tracks = tracks
    # everything together
    out = tmp_path / "all.bam"
    with _knobs(THM_BAM_SORT=1, THM_BAM_INDEX=1, THM_QUANT=1, THM_COVERAGE=3):
        capi.align_files(a, [fq], out, capi.FMT_BAM, batch_reads=700, n_threads=4)
    bam = out.read_bytes()
    data = bc.oracle_records(t, rs, r)[0]
    stream = sc.sorted_stream(data, n_sq)
    assert gzip.decompress(bam) == sc.sorted_header_bytes(t) + stream and bam.endswith(zc.EOF_BLOCK)
    wr = capi.Writer(w.ix, capi.FMT_BAM)
    header = wr.header_sorted()
    wr.close()
    assert bam.startswith(header)
    at = [len(header)]
    while at[-1] < len(bam) - len(zc.EOF_BLOCK):
        at.append(at[-1] + struct.unpack_from("<H", bam, at[-1] + 16)[0] + 1)
    assert zc.check_blocks(bam[at[0]: at[-1]])[0] == stream
    bai = (tmp_path / "all.bam.bai").read_bytes()
    assert bai == xc.expected_bai(stream, n_sq, np.diff(at).tolist(), at[0])
    index = xc.parse_bai(bai)
    with_records = {xc.fields(x)[0] for x in xc.split_records(stream)} - {-1}
    assert len(index["refs"]) == n_sq and 0 < len(with_records) < n_sq
    for s in set(range(n_sq)) - with_records:      # the references that got no record have empty sections
        assert index["refs"][s]["bins"] == [] and index["refs"][s]["ioffset"] == [] and index["refs"][s]["pseudo"] is None, s
    xc.check_queries(index, bam, stream, n_sq, xc.regions_of(stream, n_sq)[::6])
    assert ((tmp_path / "all.bam.genes.tsv").read_text(), (tmp_path / "all.bam.junctions.tsv").read_text()) == want_tables
    tracks = {p.name[len("all.bam.cov."): -len(".bedgraph")]: p.read_text() for p in tmp_path.glob("all.bam.cov.*.bedgraph")}
    assert tracks == want_tracks
    a.close()
    a2.close()
