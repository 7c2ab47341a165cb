"""What the coverage tracks of a run must hold (include/thermite_io.h, above thm_coverage_create), written from that
contract alone: `Expect` deposits the blocks of a view (offsets, records, digests, words -- the tuples of quant_common.py)
into per-base arrays with np.add.at on the block ends, takes the cumulative sum and cuts it into runs; `sam_depth` counts a
SAM file a second, independent way -- line by line from POS, the CIGAR text, the flag and NH, a slice of bases at a time.
Nothing here touches the library under test."""
import re

import numpy as np

import cigar_common as cc
import quant_common as qc
from oracle import aln_writer as ow
from thermite_amd import capi

STRANDED, MULTI = 1, 2
RUN_DT = np.dtype([("ref_id", "<u4"), ("depth", "<u4"), ("start", "<u8"), ("end", "<u8")])
TOTAL_NAMES = ["n_reads", "n_failed_reads", "n_alns", "n_skipped_multi", "n_long_run_alns"]
TRACK_TOTAL_NAMES = ["n_alns", "n_blocks", "n_bases"]
M, I, D, N, S = 0, 1, 2, 3, 4
ALL_FLAGS = (0, STRANDED, MULTI, STRANDED | MULTI)


def sq_lengths(t):
    """the LN of every @SQ line of the oracle's SAM header, in order"""
    return [int(ln.split("\t")[2][3:]) for ln in ow.sam_header(t).decode().splitlines() if ln.startswith("@SQ")]


def n_strands(flags):
    return 2 if flags & STRANDED else 1


def n_tracks(flags):
    return n_strands(flags) * (2 if flags & MULTI else 1)


def track_names(flags):
    """the <track> of the driver's <output>.cov.<track>.bedgraph files, in track order"""
    strands = [".fwd", ".rev"] if flags & STRANDED else [""]
    return [c + s for c in (["unique", "multi"] if flags & MULTI else ["unique"]) for s in strands]


def track_of(flags, multi, forward):
    """the track of an alignment, or None"""
    if multi and not flags & MULTI:
        return None
    return (1 if multi else 0) * n_strands(flags) + (1 if flags & STRANDED and not forward else 0)


def blocks_of(words, ystart):
    """[(start, end)] of the maximal stretches that consecutive M / D words cover"""
    pos = begin = int(ystart)
    out = []
    for w in words:
        n, code = int(w) >> 4, int(w) & 15
        if code in (M, D):
            pos += n
        elif code == N:
            if pos > begin:
                out.append((begin, pos))
            pos += n
            begin = pos
    if pos > begin:
        out.append((begin, pos))
    return out


def runs_of_depth(depth, ref_id):
    """the maximal intervals of equal, non-zero depth of one contig -> RUN_DT"""
    d = np.asarray(depth, np.int64)
    edge = np.flatnonzero(np.diff(np.concatenate([[0], d, [0]])) != 0)
    out = np.zeros(max(len(edge) - 1, 0), RUN_DT)
    if len(out):
        out["ref_id"], out["start"], out["end"], out["depth"] = ref_id, edge[:-1], edge[1:], d[edge[:-1]]
    return out[out["depth"] != 0]


class Expect:
    """the tracks of an object created with `flags` over the tables `t`, and its totals"""

    def __init__(self, t, flags):
        self.t, self.flags, self.lens, self.sq = t, flags, sq_lengths(t), qc.ref_sq(t)
        self.diff = [[np.zeros(n + 1, np.int64) for n in self.lens] for _ in range(n_tracks(flags))]
        self.totals = self._zero()

    @staticmethod
    def _zero():
        tot = dict.fromkeys(TOTAL_NAMES, 0)
        tot["track"] = [dict.fromkeys(TRACK_TOTAL_NAMES, 0) for _ in range(4)]
        return tot

    def add(self, offsets, alns, dig, words, status=None):
        """-> the batch's totals"""
        tot = self._zero()
        offsets = [int(x) for x in offsets]
        n_reads = max(len(offsets) - 1, 0)
        tot["n_reads"] = n_reads
        if status is not None:
            tot["n_failed_reads"] = int((np.asarray(status) != 0).sum())
        ends = [[([], []) for _ in self.lens] for _ in self.diff]
        words = np.asarray(words)
        for r in range(n_reads):
            multi = offsets[r + 1] - offsets[r] > 1
            for a in range(offsets[r], offsets[r + 1]):
                al, d = alns[a], dig[a]
                tot["n_alns"] += 1
                k = track_of(self.flags, multi, int(al["strand"]) == 1)
                if k is None:
                    tot["n_skipped_multi"] += 1
                    continue
                if int(d["flags"]) & cc.LONG_RUN:
                    tot["n_long_run_alns"] += 1
                    continue
                o, s = int(d["cigar_off"]), self.sq[int(al["ref_id"])]
                blocks = blocks_of(words[o: o + int(d["n_cigar"])], al["ystart"])
                tt = tot["track"][k]
                tt["n_alns"] += 1
                tt["n_blocks"] += len(blocks)
                for b, e in blocks:
                    assert e <= self.lens[s], "a block beyond its contig"
                    tt["n_bases"] += e - b
                    ends[k][s][0].append(b)
                    ends[k][s][1].append(e)
        for k in range(len(self.diff)):
            for s in range(len(self.lens)):
                np.add.at(self.diff[k][s], np.array(ends[k][s][0], np.int64), 1)
                np.add.at(self.diff[k][s], np.array(ends[k][s][1], np.int64), -1)
        self._sum(self.totals, tot)
        return tot

    @staticmethod
    def _sum(into, tot, k=1):
        for f in TOTAL_NAMES:
            into[f] += k * tot[f]
        for a, b in zip(into["track"], tot["track"]):
            for f in TRACK_TOTAL_NAMES:
                a[f] += k * b[f]

    def depth(self, track, s):
        d = np.cumsum(self.diff[track][s])
        assert d[-1] == 0 and d.min() >= 0
        return d[:-1].astype(np.uint32)

    def runs(self, track, first_ref=0, n_refs=None):
        n_refs = len(self.lens) - first_ref if n_refs is None else n_refs
        parts = [runs_of_depth(self.depth(track, s), s) for s in range(first_ref, first_ref + n_refs)]
        return np.concatenate(parts) if parts else np.zeros(0, RUN_DT)

    def scaled(self, k):
        out = Expect(self.t, self.flags)
        out.diff = [[d * k for d in tr] for tr in self.diff]
        self._sum(out.totals, self.totals, k)
        return out


def from_oracle(t, flags, result, status=None):
    dig, words = cc.expected_alignments(result.alns, result.ops)
    e = Expect(t, flags)
    e.add(result.offsets, result.alns, dig, words, status)
    return e


def assert_runs_equal(got, exp, what=""):
    assert len(got) == len(exp), (what, len(got), len(exp), got[:5], exp[:5])
    for f in RUN_DT.names:
        bad = np.nonzero(got[f] != exp[f])[0]
        assert len(bad) == 0, "%s run %d %s: got %s expected %s" % (what, bad[0], f, got[bad[0]], exp[bad[0]])
    assert np.ascontiguousarray(got, RUN_DT).tobytes() == np.ascontiguousarray(exp, RUN_DT).tobytes(), what


def check_result(res, exp, track, first_ref=0, n_refs=None, what=""):
    """a capi.CoverageResult against the expectation: the runs, and what the view says about them"""
    runs = exp.runs(track, first_ref, n_refs)
    assert_runs_equal(res.runs, runs, "%s track %d" % (what, track))
    length = runs["end"].astype(np.int64) - runs["start"].astype(np.int64)
    assert res.n_covered == int(length.sum()) and res.n_bases == int((length * runs["depth"]).sum()), what
    assert res.max_depth == (int(runs["depth"].max()) if len(runs) else 0), what
    assert res.totals == exp.totals, (what, res.totals, exp.totals)
    if first_ref == 0 and n_refs in (None, len(exp.lens)):
        assert res.n_bases == exp.totals["track"][track]["n_bases"], what


def check_invariants(exp):
    tot = exp.totals
    assert tot["n_alns"] == sum(x["n_alns"] for x in tot["track"]) + tot["n_skipped_multi"] + tot["n_long_run_alns"]
    for k in range(n_tracks(exp.flags)):
        runs = exp.runs(k)
        key = [(int(r["ref_id"]), int(r["start"])) for r in runs]
        assert key == sorted(key) and (runs["end"] > runs["start"]).all() and (runs["depth"] > 0).all()
        assert all(int(r["end"]) <= exp.lens[int(r["ref_id"])] for r in runs)
        # maximal: two abutting runs of one contig differ in depth
        same = (runs["ref_id"][1:] == runs["ref_id"][:-1]) & (runs["start"][1:] == runs["end"][:-1])
        assert (runs["depth"][1:][same] != runs["depth"][:-1][same]).all()
        assert int(((runs["end"] - runs["start"]) * runs["depth"].astype(np.uint64)).sum()) == tot["track"][k]["n_bases"]
    for k in range(n_tracks(exp.flags), 4):
        assert not any(tot["track"][k].values())


def table(runs, ref_id):
    """[(start, end, depth)] of one contig"""
    return [(int(r["start"]), int(r["end"]), int(r["depth"])) for r in runs if int(r["ref_id"]) == ref_id]


# ------------------------------------------------------------------ tests/golden/test_query.sam (config 1, 10 reads), counted by hand
# refIDs: some_ref 0, another_seq 1, introns_seq 2, introns_revcomp 3
GOLDEN_UNIQUE = {2: [(5, 7, 3), (7, 8, 4), (12, 16, 2), (20, 24, 4)], 3: [(5, 8, 2), (12, 16, 2), (20, 23, 2)], 1: [(8, 12, 1)], 0: []}
GOLDEN_UNIQUE_STRAND = {2: 0, 3: 1, 1: 1}     # with STRANDED: introns_seq forward, the other two reverse
GOLDEN_MULTI = {0: (0, [(2, 5, 1)]), 3: (1, [(5, 8, 1)])}   # refID -> (strand_idx, runs)


def assert_golden(t, flags, runs_of_track, totals):
    """runs_of_track(k) -> RUN_DT of all contigs; totals: of the object"""
    assert qc.sq_names(t) == ["some_ref", "another_seq", "introns_seq", "introns_revcomp"] and sq_lengths(t)[1] == 12
    ns = n_strands(flags)
    for s, want in GOLDEN_UNIQUE.items():
        for strand_idx in range(ns):
            mine = ns == 1 or GOLDEN_UNIQUE_STRAND.get(s) == strand_idx
            assert table(runs_of_track(strand_idx), s) == (want if mine else []), (flags, s, strand_idx)
    assert sum(totals["track"][k]["n_bases"] for k in range(ns)) == 58 == 34 + 20 + 4
    assert sum(totals["track"][k]["n_alns"] for k in range(ns)) == 7
    if flags & MULTI:
        for s in range(4):
            for strand_idx in range(ns):
                si, want = GOLDEN_MULTI.get(s, (0, []))
                mine = ns == 1 or si == strand_idx
                assert table(runs_of_track(ns + strand_idx), s) == (want if mine else []), (flags, s, strand_idx)
        assert sum(totals["track"][ns + k]["n_bases"] for k in range(ns)) == 6 and totals["n_skipped_multi"] == 0
    else:
        assert totals["n_skipped_multi"] == 2
    assert (totals["n_reads"], totals["n_failed_reads"], totals["n_alns"], totals["n_long_run_alns"]) == (10, 0, 9, 0)


# ------------------------------------------------------------------ SAM files
def sam_view(path, t):
    """quant_common.sam_view with thm_aln::strand from the flag"""
    off, alns, dig, words = qc.sam_view(path, t)
    flags = [f for _, f, _, _, _, _ in qc._sam_records(path) if not f & 4]
    alns["strand"] = [0 if f & 0x10 else 1 for f in flags]
    return off, alns, dig, words


def sam_depth(path, t, flags):
    """The second way: every record line on its own, a slice of bases at a time -- POS, the CIGAR text cut at its N runs, flag
    0x10 and the NH tag.  -> depth[track][refID] as int64 arrays"""
    names, lens = qc.sq_names(t), sq_lengths(t)
    depth = [[np.zeros(n, np.int64) for n in lens] for _ in range(n_tracks(flags))]
    for q, flag, rname, pos, cigar, tags in qc._sam_records(path):
        if flag & 4:
            continue
        k = track_of(flags, int(tags["NH"]) > 1, not flag & 0x10)
        if k is None:
            continue
        at = pos - 1
        for piece in re.split(r"(\d+N)", cigar):
            span = sum(int(n) for n, c in re.findall(r"(\d+)([MDN])", piece))
            if not piece.endswith("N"):
                depth[k][names.index(rname)][at: at + span] += 1
            at += span
    return depth


def bedgraph(names, depth_of_contig):
    """the text of one track's file: depth_of_contig[s] is the depth array of contig s"""
    out = []
    for s, name in enumerate(names):
        for r in runs_of_depth(depth_of_contig[s], s):
            out.append("%s\t%d\t%d\t%d\n" % (name, int(r["start"]), int(r["end"]), int(r["depth"])))
    return "".join(out)


# ------------------------------------------------------------------ the model program's input
def model_input(t, flags, views, windows=()):
    """what tests/cpp/coverage_model_main.cpp reads: the layout, the windows (track, refID, start, n) and the views, each
    added in turn"""
    lens, sq = sq_lengths(t), qc.ref_sq(t)
    parts = [np.array([flags, len(sq), len(lens), len(windows), len(views)], "<u8"), np.array(sq, "<i4"), np.array(lens, "<u8"),
             np.array(list(windows), "<u8").reshape(-1)]
    for offsets, alns, dig, words, *rest in views:
        status = rest[0] if rest else None
        offsets = np.ascontiguousarray(offsets, "<u8")
        if len(offsets) == 0:
            offsets = np.zeros(1, "<u8")
        parts += [np.array([len(offsets) - 1, len(alns), len(words), 0 if status is None else 1], "<u8"), offsets,
                  np.ascontiguousarray(alns, capi.ALN_DT), np.ascontiguousarray(dig, cc.DIGEST_DT), np.ascontiguousarray(words, "<u4")]
        if status is not None:
            parts.append(np.ascontiguousarray(status, "<i4"))
    return b"".join(p.tobytes() for p in parts)


def model_output(flags, windows, out):
    """-> (totals dict, [runs per track], [depths per window])"""
    tot_w = np.frombuffer(out[:136], "<u8")
    tot = {k: int(v) for k, v in zip(TOTAL_NAMES, tot_w)}
    tot["track"] = [{f: int(tot_w[5 + 3 * k + j]) for j, f in enumerate(TRACK_TOTAL_NAMES)} for k in range(4)]
    at, runs, depths = 136, [], []
    for _ in range(n_tracks(flags)):
        n = int(np.frombuffer(out[at: at + 8], "<u8")[0])
        runs.append(np.frombuffer(out[at + 8: at + 8 + 24 * n], RUN_DT))
        at += 8 + 24 * n
    for _, _, _, n in windows:
        depths.append(np.frombuffer(out[at: at + 4 * n], "<u4"))
        at += 4 * n
    assert at == len(out)
    return tot, runs, depths


# ------------------------------------------------------------------ views made by hand (the add_view shapes)
CONTIG = 300000


def shape_tables():
    """three contigs made for the shapes: two of 300 000 bases, so that a block can span several tiles, and one of 1000
    between them, which a block can cover whole"""
    from thermite_amd import refdata
    rng = np.random.default_rng(418)
    seq = lambda n: np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]
    genes = [dict(id="COVG%d" % g, name="cov%d" % g) for g in range(2)]
    txs = [dict(id="COVT0", gene_idx=0, chrom="cov_a", strand=True, exons=[(1000, 1400), (2000, 2300)]),
           dict(id="COVT1", gene_idx=1, chrom="cov_b", strand=False, exons=[(5000, 5600)])]
    return refdata.build_tables([("cov_a", seq(CONTIG)), ("cov_small", seq(1000)), ("cov_b", seq(CONTIG))], genes, txs)


def ref_of(t, s, forward=True):
    """a thm_ref index of @SQ entry s"""
    sq = qc.ref_sq(t)
    return [r for r in range(len(sq)) if sq[r] == s and bool(t["refs"][r]["strand"]) == forward][0]


def make_view(reads):
    """quant_common.make_view over alignments dict(ref_id, ystart, cigar | long_run, strand=1): exonic on transcript 0"""
    off, alns, dig, words = qc.make_view([[dict(a, aln_type=qc.EXONIC, idx=0) for a in r] for r in reads])
    if len(alns):
        alns["strand"] = [a.get("strand", 1) for r in reads for a in r]
    return off, alns, dig, words


def uniform_view(n_reads, alns_per_read, ref_id, ystart, cigar, strand=1):
    off, alns, dig, words = qc.uniform_view(n_reads, alns_per_read, ref_id, ystart, 0, cigar)
    alns["strand"] = strand
    return off, alns, dig, words


def shape_cases(t, tile):
    """name -> list of views (each added in turn) over shape_tables(); `tile` is the tile size of the fetch kernels"""
    a, small, b = ref_of(t, 0), ref_of(t, 1), ref_of(t, 2)
    a_rev = ref_of(t, 0, False)
    assert sq_lengths(t) == [CONTIG, 1000, CONTIG] and tile <= 65536
    many = [(3, "S"), (7, "M")]
    for k in range(40):
        many += [(100 + k, "N")]
        if k == 17:
            many += [(90, "N")]                    # two adjacent N words: no block between them
        many += [(2, "M"), (1, "I"), (1 + k % 3, "M"), (2, "D"), (k % 5, "M")] if k % 2 else [(4 + k, "M")]
    many += [(2, "S")]
    assert sum(1 for _, c in many if c == "N") == 41
    one = lambda ref, at, cigar, **kw: [dict(ref_id=ref, ystart=at, cigar=cigar, **kw)]
    edges = sorted({p for m in (65536, tile, 2 * tile, 3 * tile) for p in (m - 1, m, m + 1)})
    edge_reads = [one(a, s, [(e - s, "M")]) for s in edges for e in edges if e > s]
    edge_reads += [one(b, 0, [(p, "M")]) for p in edges] + [one(b, p, [(CONTIG - p, "M")]) for p in edges]
    return {
        "empty": [make_view([])],
        "no_alignments": [make_view([[], [], []])],
        "whole_contig": [make_view([one(small, 0, [(1000, "M")]), one(b, 0, [(50, "M")]), one(a, CONTIG - 30, [(30, "M")])])],
        "abutting": [make_view([one(a, 100, [(10, "M")]), one(a, 110, [(10, "M")])])],
        "tile_span": [make_view([one(a, 20000, [(250000, "M")]), one(a, 140000, [(100, "M")])])],
        "tile_edge": [make_view(edge_reads)],
        "hot": [uniform_view(70000, 1, b, 123456, [(50, "M")])],
        "forty_introns": [make_view([one(a, 5000, many), [], one(a, 5000, many) + one(a_rev, 5010, many[1:], strand=0)])],
        "one_read_5000": [uniform_view(1, 5000, a, 1000, [(30, "M"), (500, "N"), (61, "M")])],
        "both_strands": [make_view([one(a, 7000, [(91, "M")]), one(a_rev, 7040, [(91, "M")], strand=0), one(b, 7000, [(20, "M"), (9, "N"), (5, "M")], strand=0)])],
        "long_run": [make_view([[dict(ref_id=a, ystart=100, long_run=True)], one(a, 100, [(30, "M"), (500, "N"), (61, "M")])])],
        "later_add": [make_view([one(a, 9000, [(100, "M")]), one(b, 50, [(91, "M")])]),
                      make_view([one(a, 9040, [(20, "M")]), one(a, 9100, [(10, "M")])]),
                      make_view([one(a, 8990, [(10, "M"), (2, "D"), (8, "M"), (3, "I"), (30, "M")])])],
    }


def assert_shape(name, flags, e, tile):
    """what each shape is there for, on the expectation"""
    tot = e.totals
    if name == "whole_contig":
        assert table(e.runs(0), 1) == [(0, 1000, 1)] and table(e.runs(0), 2) == [(0, 50, 1)] and table(e.runs(0), 0) == [(CONTIG - 30, CONTIG, 1)]
    if name == "abutting":
        assert table(e.runs(0), 0) == [(100, 120, 1)] and tot["track"][0]["n_blocks"] == 2
    if name == "tile_span":
        assert table(e.runs(0), 0) == [(20000, 140000, 1), (140000, 140100, 2), (140100, 270000, 1)]
        assert all(r[1] // tile - r[0] // tile >= 3 for r in table(e.runs(0), 0)[::2])
    if name == "tile_edge":
        starts = set(e.runs(0)["start"].tolist()) | set(e.runs(0)["end"].tolist())
        assert {m + d for m in (65536, tile, 2 * tile, 3 * tile) for d in (-1, 0, 1)} <= starts
    if name == "hot":
        assert table(e.runs(0), 2) == [(123456, 123506, 70000)] and tot["track"][0]["n_bases"] == 3500000
    if name == "forty_introns":
        assert tot["n_alns"] == 3 and sum(x["n_blocks"] for x in tot["track"]) + (0 if flags else 41 * 2) == 41 * 3
    if name == "one_read_5000":
        if flags:
            k = n_strands(flags)
            assert table(e.runs(k), 0) == [(1000, 1030, 5000), (1530, 1591, 5000)] and tot["track"][0]["n_alns"] == 0
        else:
            assert tot["n_skipped_multi"] == 5000 and len(e.runs(0)) == 0
    if name == "both_strands":
        if flags:
            assert table(e.runs(0), 0) == [(7000, 7091, 1)] and table(e.runs(1), 0) == [(7040, 7131, 1)]
            assert table(e.runs(1), 2) == [(7000, 7020, 1), (7029, 7034, 1)]
        else:
            assert table(e.runs(0), 0) == [(7000, 7040, 1), (7040, 7091, 2), (7091, 7131, 1)]
    if name == "long_run":
        assert tot["n_long_run_alns"] == 1 and tot["track"][0]["n_alns"] == 1 and tot["track"][0]["n_blocks"] == 2
    if name == "later_add":
        # the first view alone is (9000, 9100, 1): the later ones deepen its head, lengthen it and split it
        assert table(e.runs(0), 0) == [(8990, 9000, 1), (9000, 9060, 2), (9060, 9110, 1)] and table(e.runs(0), 2) == [(50, 141, 1)]


def shape_windows(tile):
    """(track, refID, start, n) windows of thm_coverage_depth for the shapes: mid-tile starts, a contig's last base, n = 1"""
    return [(0, 0, 0, 1), (0, 0, 8990, 200), (0, 0, tile - 3, 2 * tile + 7), (0, 0, CONTIG - 40, 40), (0, 1, 0, 1000), (0, 1, 999, 1),
            (0, 2, 123400, 200), (0, 0, 65530, 10), (0, 2, 0, 60)]


def bad_views(t):
    """name -> a view that the device's pass must refuse"""
    a = ref_of(t, 0)
    good = [dict(ref_id=a, ystart=100, cigar=[(50, "M")])]
    past = make_view([good, [dict(ref_id=ref_of(t, 1), ystart=950, cigar=[(20, "M"), (10, "N"), (21, "M")])]])   # ends at 1001 of 1000
    no_sq = make_view([good, good])
    no_sq[1]["ref_id"][1] = len(t["refs"])
    pool = make_view([good, good])
    pool[2]["cigar_off"][1] = 2
    return {"past_the_contig": past, "no_refid": no_sq, "outside_the_pool": pool}
