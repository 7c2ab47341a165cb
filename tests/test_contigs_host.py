"""What tests/test_gpu_contigs.py relies on, asserted from the CPU oracle alone: the many-contig world of
tests/contigs_common.py and its reads do reach the code that only a reference of many contigs reaches -- several
contig-copy boundaries inside one bin of idx_to_ref, alignments that overlap on different contigs, contig names whose
byte order is not the file order, windows clamped at both ends of short contigs.  The floors are conditions on the inputs,
so that no GPU case can pass with its path idle."""
import numpy as np
import pytest

import bam_common as bc
import contigs_common as cg
import smem_finish_common as sf
from gpu_common import TEAM_HITS, World
from oracle import pyoracle as orc
from thermite_amd import capi, refdata

_memo = {}


def _w():
    if "w" not in _memo:
        _memo["w"] = World(cg.world()[0])
    return _memo["w"]


def _run():
    """the general read set through the oracle, once: (bases, offsets, result, per-alignment read, per-alignment contig)"""
    if "run" not in _memo:
        w = _w()
        bases, off = cg.pack(cg.read_set())
        r = w.oix.align_batch(bases, off, capi.CI_OPTS, n_threads=8)
        n_alns = np.diff(r.offsets.astype(np.int64))
        _memo["run"] = (bases, off, r, np.repeat(np.arange(len(n_alns)), n_alns), cg.contig_of(w.t, r.alns["ref_id"]))
    return _memo["run"]


def _per_read(r):
    o = r.offsets.astype(np.int64)
    return [(i, slice(int(o[i]), int(o[i + 1]))) for i in range(len(o) - 1) if o[i + 1] - o[i] >= 2]


# ------------------------------------------------------------------ the world
def test_the_world_is_what_the_issue_asks_for():
    t, info = cg.world()
    lens, kind, names = info["lens"], info["kind"], t["names"]
    assert 250_000 <= len(t["text"]) <= 400_000 and len(t["refs"]) == 2 * len(lens)
    assert names != sorted(names, key=str.encode) and len(set(names)) == len(names)
    assert not np.array_equal(np.argsort(t["name_rank"]), np.arange(len(names)))
    assert ((lens >= 15000) & (lens <= 40000)).sum() >= 3 and ((lens >= 400) & (lens <= 5000)).sum() >= 6
    short = lens[(lens >= 30) & (lens <= 1500)]
    assert len(short) >= 40 and {90, 91, 92} <= set(short.tolist())
    assert {1, 2, cg.K - 1, cg.K} <= set(lens.tolist())
    # a run of consecutive contigs of at most 80 bases: their copies put more than ten boundaries into one bin
    run = np.nonzero(kind == "tiny")[0]
    assert len(run) >= 12 and np.array_equal(run, np.arange(run[0], run[0] + len(run))) and lens[run].max() <= 80
    refs = t["refs"][2 * run[0]: 2 * (run[-1] + 1)]
    in_bin = np.bincount((refs["end_idx"].astype(np.int64) >> cg.GRID_SHIFT))
    assert in_bin.max() > 10
    # N runs: a leading and a trailing one, an interior one, a contig that is N throughout
    f = {n: cg.forward(t, info["index_of"][n]) for n in ("chr10", "MT", "chr1", cg.SCAF_ALL_N)}
    assert (f["chr10"][:500] == ord("N")).all() and (f["MT"][-400:] == ord("N")).all() and (f[cg.SCAF_ALL_N] == ord("N")).all()
    a, b = info["n_runs"]["chr1"]
    assert 0 < a and b < len(f["chr1"]) and (f["chr1"][a:b] == ord("N")).all() and f["chr1"][a - 1] != ord("N")
    # paralogs: the segment at one coordinate of six contigs (three exact, one reverse-complemented, two diverged)
    seg = [cg.forward(t, info["index_of"][n])[cg.P1_AT: cg.P1_AT + cg.P1_LEN] for n, _ in cg.LARGE]
    assert cg.P1_LEN >= 1200 and all(np.array_equal(s, info["p1"]) for s in seg[:3]) and np.array_equal(seg[3], refdata.revcomp(info["p1"]))
    assert all(0.005 < (s != info["p1"]).mean() < 0.04 for s in seg[4:])
    for fam, n in (("F2", 24), ("F4", 12)):
        pl = info["plants"][fam]
        assert len(pl) == n and len({c for c, _, _ in pl}) >= 6 and {f for _, _, f in pl} == {True, False}
        for c, at, fwd in pl:
            u = cg.forward(t, info["index_of"][c])[at: at + cg.FAM_LEN]
            assert np.array_equal(u if fwd else refdata.revcomp(u), info["fam"][fam])
    assert len(info["plants"]["F3"]) >= 300 and len({c for c, _, _ in info["plants"]["F3"]}) >= 6
    (c, at, fwd), = info["plants"]["whole91"]
    u = cg.forward(t, info["index_of"][c])[at: at + 91]
    assert c == "chr2" and np.array_equal(u if fwd else refdata.revcomp(u), cg.forward(t, info["index_of"][cg.SCAF_WHOLE_91]))
    # annotation: genes flush with contig ends on each strand, a gene that is a whole contig, a transcript and its contig
    # shorter than a read, an exon inside the paralogous segment, contigs without a gene
    tc = info["tx_contig"]
    assert len(np.unique(tc[: -len(info["hand"])])) >= 4 and len(set(t["tx_ids"])) == len(t["tx_ids"]) and len(set(t["gene_ids"])) == len(t["gene_ids"])
    ends = set()
    for key in ("first_fwd", "last_rev", "last_fwd", "first_rev"):
        tx = t["txs"][info["hand"][key]["tx"]]
        ex = t["exons"][int(tx["exon_begin"]): int(tx["exon_begin"]) + int(tx["n_exons"])]
        ref = t["refs"][orc_idx_to_ref(t, int(ex["start"][0]))]
        at_start, at_end = int(ex["start"][0]) == int(ref["start_idx"]), int(ex["end"][-1]) == int(ref["end_idx"]) - 1
        assert at_start or at_end
        # (a '-' gene lies on the reverse copy: its first exon in text order is the contig's last)
        fwd = bool(tx["strand"])
        ends.add((fwd, "first base" if at_start == fwd else "last base"))
    assert ends == {(True, "first base"), (True, "last base"), (False, "first base"), (False, "last base")}
    assert lens[info["index_of"][cg.SCAF_GENE_300]] == 300 and int(t["txs"][info["hand"]["whole_contig"]["tx"]]["seq_len"]) == 300
    assert lens[info["index_of"][cg.SCAF_SHORT_TX]] < cg.L0 and int(t["txs"][info["hand"]["short_tx"]["tx"]]["seq_len"]) < cg.L0
    assert len(set(range(len(lens))) - set(tc.tolist())) >= 40


def orc_idx_to_ref(t, idx):
    return int(np.searchsorted(t["refs"]["end_idx"], idx, side="right"))


def test_the_smallest_contigs_are_taken_by_index_builder_and_oracle():
    """1, 2, k - 1 and k bases: neither refuses a length, so all four stay in the world; each is found by idx_to_ref"""
    w = _w()
    for n in cg.SMALLEST:
        ci = cg.world()[1]["index_of"]["z%d" % n]
        for copy in (2 * ci, 2 * ci + 1):
            r = w.t["refs"][copy]
            assert int(r["len"]) == n
            for idx in (int(r["start_idx"]), int(r["end_idx"]) - 1):
                assert w.ix.idx_to_ref(idx)[0] == copy == orc_idx_to_ref(w.t, idx)


def test_simulate_reads_with_an_intronic_fraction_is_not_for_this_world():
    """synth.simulate_reads draws its genomic windows from any contig copy, shorter than a read or not: on this world it
    reads across '$' into the next copy (and would run off the text, were the last contig a short one).  The reads of this
    world come from contigs_common's own maker, which stays inside a contig."""
    from thermite_amd import synth
    t = cg.world()[0]
    bases, _, _ = synth.simulate_reads(t, 2000, 91, intronic_frac=0.5)
    assert (bases == ord("$")).any()
    assert not any(b"$" in s for s in cg.read_set()["seqs"])


# ------------------------------------------------------------------ the reads
def test_the_read_sets():
    rs = cg.read_set()
    lens = np.array([len(s) for s in rs["seqs"]])
    assert 4000 <= len(lens) <= 6000 and lens.min() == 0 and lens.max() == 300 and len(set(lens.tolist())) > 150
    n_count = np.array([s.count(b"N") for s in rs["seqs"]])
    kinds = np.array(rs["kinds"])
    assert (n_count[kinds != "n_run"] <= 1).all() and (n_count == 1).sum() >= 100 and (kinds == "n_run").sum() == 2
    want = {"tx", "genomic", "p1_91", "p1_150", "p1_300", "F2", "F3", "F4", "end_tail", "end_head", "end_whole", "end_equal", "end_join",
            "fin_E", "fin_S", "ragged", "random", "n_run"}
    assert want <= set(rs["kinds"])
    for name in ("list", "team", "wide", "per_hit", "tiny"):
        assert 8 <= len(cg.read_set(name)["seqs"]) <= 600, name
    # the two reads with a run of N stay cheap
    w = _w()
    bases, off = refdata.pack_reads([s for s, k in zip(rs["seqs"], rs["kinds"]) if k == "n_run"])
    hits = np.diff(w.oix.all_smems(sf.sanitise(bases), off, cg.K).offsets.astype(np.int64))
    assert (hits >= 1).all() and (hits <= 4).all(), hits


def test_no_read_where_the_reference_would_panic():
    assert _run()[2].counters[15] == 0
    w = _w()
    for name, opts in (("list", capi.CI_OPTS), ("team", capi.CI_OPTS), ("wide", cg.WIDE_OPTS), ("per_hit", capi.CI_OPTS), ("tiny", cg.TINY_OPTS)):
        bases, off = cg.pack(cg.read_set(name))
        assert w.oix.align_batch(bases, off, opts, n_threads=8).counters[15] == 0, name


def test_overlapping_alignments_on_different_contigs_survive():
    """filter_overlapping (src/aligner.rs:322-346) restarts its sweep when the name changes: two alignments whose
    [ystart, yend) overlap, on different contigs, are both kept"""
    bases, off, r, read_of, contig = _run()
    n = 0
    for i, s in _per_read(r):
        a, c = r.alns[s], contig[s]
        ys, ye = a["ystart"].astype(np.int64), a["yend"].astype(np.int64)
        over = (ys[:, None] < ye[None, :]) & (ys[None, :] < ye[:, None]) & (c[:, None] != c[None, :])
        n += bool(over.any())
    assert n >= 100, n


def test_equal_scores_come_out_in_name_order_not_file_order():
    bases, off, r, read_of, contig = _run()
    n = 0
    for i, s in _per_read(r):
        a, c = r.alns[s], contig[s]
        best = c[a["score"] == a["score"].max()]
        n += bool((np.diff(best) < 0).any())
    assert n >= 50, n


def test_more_alignments_than_the_register_path_keeps():
    bases, off, r, read_of, contig = _run()
    n = sum(1 for i, s in _per_read(r) if s.stop - s.start > cg.KEYCAP and len(set(contig[s].tolist())) >= 3)
    assert n >= 20, n
    # the dedicated read set: the same, for most of its reads
    w = _w()
    lb, lo = cg.pack(cg.read_set("list"))
    rl = w.oix.align_batch(lb, lo, capi.CI_OPTS, n_threads=8)
    assert (np.diff(rl.offsets.astype(np.int64)) > cg.KEYCAP).sum() >= 40


def test_team_and_heavy_hit_counts_over_several_contigs():
    w = _w()
    for name in ("general", "team"):
        bases, off = cg.pack(cg.read_set(name))
        m = w.oix.all_smems(sf.sanitise(bases), off, cg.K)
        mo = m.offsets.astype(np.int64)
        hits = np.diff(mo)
        on = [len(set(cg.contig_of(w.t, [orc_idx_to_ref(w.t, int(x)) for x in m.mems["ref_idx"][mo[i]: mo[i + 1]]]).tolist())) for i in range(len(hits))]
        on = np.array(on)
        assert ((hits >= TEAM_HITS) & (on >= 3)).sum() >= 4, name
        assert ((hits >= 8) & (hits < 32) & (on >= 3)).sum() >= 4, name


def test_alignments_on_short_contigs_and_at_contig_ends():
    bases, off, r, read_of, contig = _run()
    t, info = cg.world()
    lens, a = info["lens"], r.alns
    assert (lens[contig] < 1024).sum() >= 50
    assert (info["kind"][contig] == "tiny").sum() >= 20
    clipped = ((a["ystart"] == 0) | (a["yend"] == a["ylen"])) & ((a["xstart"] > 0) | (a["xend"] < a["xlen"]))
    assert clipped.sum() >= 20
    assert np.array_equal(a["ylen"].astype(np.int64), lens[contig])
    exonic = a["aln_type"] == 0
    gene = t["txs"]["gene_idx"][a["tx_or_gene_idx"][exonic]]
    assert np.isin(gene, info["edge_genes"]).sum() >= 10
    for g in info["edge_genes"]:
        assert (gene == g).sum() >= 2, g
    assert (a["tx_or_gene_idx"][exonic] == info["hand"]["short_tx"]["tx"]).sum() >= 1
    assert (gene == info["hand"]["whole_contig"]["gene"]).sum() >= 1
    # the read from the exon inside the paralogous segment: exonic on one contig, not exonic on another
    both = 0
    for i, s in _per_read(r):
        ty = a["aln_type"][s]
        both += bool((ty == 0).any() and (ty == 2).any() and len(set(contig[s].tolist())) >= 2)
    assert both >= 5, both
    # every contig that can hold a seed and an alignment has one
    got = set(contig.tolist())
    for ci in range(len(lens)):
        if cg.holds_alignment(t, info, ci):
            assert ci in got, t["names"][ci]
    # ... and so do the contigs of fewer than 30 bases that can hold a seed, once the score threshold lets them
    w = _w()
    tb, to = cg.pack(cg.read_set("tiny"))
    rt = w.oix.align_batch(tb, to, cg.TINY_OPTS, n_threads=4)
    on = set(cg.contig_of(t, rt.alns["ref_id"]).tolist())
    assert info["index_of"]["z%d" % cg.K] in on
    for n in cg.SMALLEST[:-1]:   # no seed fits
        assert info["index_of"]["z%d" % n] not in on


# ------------------------------------------------------------------ idx_to_ref
@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
def test_idx_to_ref_bin_and_walk(wide):
    """the two loads and the walk every kernel restates, from the host's tables (thm_debug_host_table 0 and 1), against
    refs.partition_point(end_idx <= idx) (src/index.rs:287-290) in plain numpy"""
    t, info = cg.world()
    w = _w() if not wide else World(t, wide=True)
    ref_bin, ref_recs = cg.ref_tables(w.ix)
    assert len(ref_recs) == len(t["refs"]) and len(ref_bin) == (len(t["text"]) >> cg.GRID_SHIFT) + 1
    assert np.array_equal(ref_recs["end"], t["refs"]["end_idx"]) and np.array_equal(ref_recs["start"], t["refs"]["start_idx"])
    assert np.array_equal(ref_recs["name_rank"], t["name_rank"][t["refs"]["name_id"]])
    run = np.nonzero(info["kind"] == "tiny")[0]
    lo, hi = int(t["refs"][2 * run[0]]["start_idx"]), int(t["refs"][2 * run[-1] + 1]["end_idx"])
    rng = np.random.default_rng(5)
    idx = np.concatenate([np.arange(lo, hi), rng.integers(0, len(t["text"]), 2000), t["refs"]["end_idx"].astype(np.int64) - 1,
                          t["refs"]["start_idx"].astype(np.int64)])
    want = np.searchsorted(t["refs"]["end_idx"], idx, side="right")
    steps = 0
    for x, k in zip(idx.tolist(), want.tolist()):
        got, n = cg.bin_and_walk(ref_bin, ref_recs, x)
        assert got == k, (x, got, k)
        steps = max(steps, n)
    assert steps >= 10, steps
    # the largest walk over all bins: from a bin's first contig copy to the last one that begins in it
    last_in_bin = np.searchsorted(t["refs"]["end_idx"], (np.arange(len(ref_bin), dtype=np.int64) << cg.GRID_SHIFT) + (1 << cg.GRID_SHIFT) - 1, side="right")
    assert int((np.minimum(last_in_bin, len(ref_recs) - 1) - ref_bin).max()) >= 10


# ------------------------------------------------------------------ the finisher's host program
def test_finisher_host_program_on_later_contigs(tmp_path):
    """smem_finish.h (ref_of, the windows' clamps) over the general read set: what it finishes equals the oracle's, and
    both classes finish reads on contigs other than the first"""
    w = _w()
    exe = sf.host_program(tmp_path)
    bases, off, r, read_of, contig = _run()
    out, half = sf.run_host(exe, w, capi.CI_OPTS, bases, off, tmp_path)
    assert sf.assert_host_matches_oracle(w, capi.CI_OPTS, bases, off, out, half) > 0
    later = cg.contig_of(w.t, out["ref_id"].clip(0, len(w.t["refs"]) - 1)) != 0
    done = (out["what"] == 1) & (out["accepted"] > 0)
    e, s = int((done & later & (out["shape"] == 1)).sum()), int((done & later & (out["shape"] == 2)).sum())
    assert e >= 20 and s >= 20, (e, s)
    # among them the first and the last window of a contig
    first = done & later & (out["ystart"] == 0)
    last = done & later & (out["yend"] == out["ylen"])
    assert first.sum() >= 4 and last.sum() >= 4, (int(first.sum()), int(last.sum()))


# ------------------------------------------------------------------ the registered read set
def test_registered_with_the_bam_read_sets():
    assert "contigs" in bc.READ_SETS and bc.REF_OF["contigs"] == "contigs"
    t = bc.tables("contigs")
    rs = bc.read_set("contigs", t)
    assert t is cg.world()[0] and rs["seqs"] == cg.read_set()["seqs"] and rs["opts"] == capi.CI_OPTS
    assert len(rs["names"]) == len(rs["seqs"]) == len(rs["quals"]) and len(set(rs["names"])) == len(rs["names"])
    # @SQ order is file order, name_rank is byte order: the two disagree in this world
    from oracle import aln_writer as ow
    sq = [ln.split(b"\t")[1][3:].decode() for ln in ow.sam_header(t).splitlines() if ln.startswith(b"@SQ")]
    assert sq == t["names"] and sq != sorted(sq, key=str.encode)
