"""What the gene and junction count tables of a run must hold (include/thermite_io.h, above thm_quant_create), written from
that contract alone: `expected_tables` counts over a view (offsets, records, digests, words), `from_oracle` takes the
oracle's alignments there through cigar_common.expected_alignments, `sam_view` parses a SAM file into such a view, and
`count_sam` counts a SAM file a second, independent way -- line by line from its NH / RE / GX / TX tags, positions and
CIGAR text.  Nothing here touches the library under test."""
import re

import numpy as np

import cigar_common as cc
from oracle import aln_writer as ow
from thermite_amd import capi

TOTAL_NAMES = ["n_reads", "n_failed_reads", "n_unmapped_reads", "n_unique_reads", "n_multi_reads", "n_alns",
               "n_intergenic_unique", "n_intergenic_multi", "n_spliced_alns", "n_junction_hits", "n_long_run_alns"]
GENE_DT = np.dtype([("exonic_unique", "<u8"), ("exonic_multi", "<u8"), ("intronic_unique", "<u8"), ("intronic_multi", "<u8")])
JUNCTION_DT = np.dtype([("ref_id", "<u4"), ("strand", "<u4"), ("start", "<u8"), ("end", "<u8"), ("n_unique", "<u8"),
                        ("n_multi", "<u8"), ("max_overhang", "<u4"), ("pad", "<u4")])
EXONIC, INTRONIC, INTERGENIC = 0, 1, 2
M, I, D, N, S = 0, 1, 2, 3, 4


def sq_names(t):
    """the @SQ names of the oracle's SAM header, in order: a contig's index there is its BAM refID"""
    return [ln.split("\t")[1][3:] for ln in ow.sam_header(t).decode().splitlines() if ln.startswith("@SQ")]


def ref_sq(t):
    """per thm_ref: its BAM refID"""
    names = sq_names(t)
    return [names.index(t["names"][int(r["name_id"])]) for r in t["refs"]]


def junction_hits(words, ystart):
    """[(start, end, overhang)] of the N words of one genome CIGAR"""
    pos, anchors, hits = int(ystart), [0], []
    for w in words:
        n, code = int(w) >> 4, int(w) & 15
        if code == M:
            anchors[-1] += n
        if code == N:
            hits.append((pos, pos + n))
            anchors.append(0)
        if code in (M, D, N):
            pos += n
    return [(s, e, min(anchors[k], anchors[k + 1])) for k, (s, e) in enumerate(hits)]


def expected_tables(t, offsets, alns, dig, words, status=None):
    """-> dict(genes: GENE_DT[n_genes], junctions: JUNCTION_DT[...] sorted, totals: dict)"""
    n_genes = len(t["genes"])
    genes = np.zeros((n_genes, 4), np.uint64)
    tot = dict.fromkeys(TOTAL_NAMES, 0)
    rows = {}
    sq = ref_sq(t)
    offsets = [int(x) for x in offsets]
    for r in range(len(offsets) - 1):
        nh = offsets[r + 1] - offsets[r]
        tot["n_reads"] += 1
        if status is not None and int(status[r]) != 0:
            tot["n_failed_reads"] += 1
        elif nh == 0:
            tot["n_unmapped_reads"] += 1
        else:
            tot["n_unique_reads" if nh == 1 else "n_multi_reads"] += 1
        multi = nh > 1
        for a in range(offsets[r], offsets[r + 1]):
            al, d = alns[a], dig[a]
            tot["n_alns"] += 1
            ty, idx = int(al["aln_type"]), int(al["tx_or_gene_idx"])
            if ty == EXONIC:
                genes[int(t["txs"][idx]["gene_idx"]), 1 if multi else 0] += 1
            elif ty == INTRONIC:
                genes[idx, 3 if multi else 2] += 1
            else:
                tot["n_intergenic_multi" if multi else "n_intergenic_unique"] += 1
            if int(d["flags"]) & cc.LONG_RUN:
                tot["n_long_run_alns"] += 1
                continue
            o = int(d["cigar_off"])
            hits = junction_hits(words[o: o + int(d["n_cigar"])], al["ystart"])
            if hits:
                assert ty == EXONIC, "an intron outside an exonic alignment"
                tot["n_spliced_alns"] += 1
                forward = bool(t["txs"][idx]["strand"])
                for s, e, ov in hits:
                    key = (sq[int(al["ref_id"])], s, e, 0 if forward else 1)
                    row = rows.setdefault(key, [0, 0, 0])
                    row[1 if multi else 0] += 1
                    row[2] = max(row[2], ov)
                    tot["n_junction_hits"] += 1
    j = np.zeros(len(rows), JUNCTION_DT)
    for k, key in enumerate(sorted(rows)):
        nu, nm, ov = rows[key]
        j[k] = (key[0], 1 - key[3], key[1], key[2], nu, nm, ov, 0)
    g = np.zeros(n_genes, GENE_DT)
    for c, f in enumerate(GENE_DT.names):
        g[f] = genes[:, c]
    return dict(genes=g, junctions=j, totals=tot)


def from_oracle(t, result, status=None):
    dig, words = cc.expected_alignments(result.alns, result.ops)
    return expected_tables(t, result.offsets, result.alns, dig, words, status)


def add_tables(a, b):
    """the tables of two runs, merged by key: counts summed, overhang maximum"""
    rows = {}
    for j in list(a["junctions"]) + list(b["junctions"]):
        key = (int(j["ref_id"]), int(j["start"]), int(j["end"]), 1 - int(j["strand"]))
        row = rows.setdefault(key, [0, 0, 0])
        row[0] += int(j["n_unique"])
        row[1] += int(j["n_multi"])
        row[2] = max(row[2], int(j["max_overhang"]))
    out = np.zeros(len(rows), JUNCTION_DT)
    for k, key in enumerate(sorted(rows)):
        out[k] = (key[0], 1 - key[3], key[1], key[2], rows[key][0], rows[key][1], rows[key][2], 0)
    g = np.zeros(len(a["genes"]), GENE_DT)
    for f in GENE_DT.names:
        g[f] = a["genes"][f] + b["genes"][f]
    return dict(genes=g, junctions=out, totals={k: a["totals"][k] + b["totals"][k] for k in TOTAL_NAMES})


def scale_tables(x, k):
    out = dict(genes=x["genes"].copy(), junctions=x["junctions"].copy(), totals={n: v * k for n, v in x["totals"].items()})
    for f in GENE_DT.names:
        out["genes"][f] *= k
    for f in ("n_unique", "n_multi"):
        out["junctions"][f] *= k
    return out


def pack(x):
    """the three results as bytes: totals, gene rows, junction rows (what the model program writes, and what a fetch holds)"""
    tot = np.array([x["totals"][k] for k in TOTAL_NAMES], "<u8")
    return tot.tobytes() + np.ascontiguousarray(x["genes"]).tobytes() + np.ascontiguousarray(x["junctions"]).tobytes()


def of_result(res):
    """a capi.QuantResult in the same form"""
    return dict(genes=res.genes, junctions=res.junctions, totals=res.totals)


def assert_tables_equal(got, exp, what=""):
    assert got["totals"] == exp["totals"], (what, got["totals"], exp["totals"])
    for f in GENE_DT.names:
        bad = np.nonzero(got["genes"][f] != exp["genes"][f])[0]
        assert len(bad) == 0, "%s gene %d %s: got %d expected %d" % (what, bad[0], f, got["genes"][f][bad[0]], exp["genes"][f][bad[0]])
    assert len(got["junctions"]) == len(exp["junctions"]), (what, len(got["junctions"]), len(exp["junctions"]))
    for f in JUNCTION_DT.names:
        bad = np.nonzero(got["junctions"][f] != exp["junctions"][f])[0]
        assert len(bad) == 0, "%s junction %d %s: got %s expected %s" % (what, bad[0], f, got["junctions"][bad[0]], exp["junctions"][bad[0]])
    assert pack(got) == pack(exp), what


def check_invariants(x):
    tot = x["totals"]
    assert tot["n_reads"] == tot["n_failed_reads"] + tot["n_unmapped_reads"] + tot["n_unique_reads"] + tot["n_multi_reads"]
    assert tot["n_alns"] == sum(int(x["genes"][f].sum()) for f in GENE_DT.names) + tot["n_intergenic_unique"] + tot["n_intergenic_multi"]
    assert tot["n_junction_hits"] == int(x["junctions"]["n_unique"].sum() + x["junctions"]["n_multi"].sum())
    key = [(int(j["ref_id"]), int(j["start"]), int(j["end"]), 1 - int(j["strand"])) for j in x["junctions"]]
    assert key == sorted(set(key))


# ------------------------------------------------------------------ tests/golden/test_query.sam (config 1, 10 reads), counted by hand
GOLDEN_GENES = {"some_ref_gene1": (0, 1, 0, 0), "another_seq_gene1": (1, 0, 0, 0), "introns_seq_gene1": (4, 0, 0, 0),
                "introns_revcomp_gene1": (2, 1, 0, 0)}
GOLDEN_JUNCTIONS = [(2, 8, 12, "+", 2, 3), (2, 8, 20, "+", 2, 3), (2, 16, 20, "+", 2, 4), (3, 8, 12, "-", 2, 3), (3, 16, 20, "-", 2, 3)]
GOLDEN_TOTALS = dict(n_reads=10, n_failed_reads=0, n_unmapped_reads=2, n_unique_reads=7, n_multi_reads=1, n_alns=9,
                     n_intergenic_unique=0, n_intergenic_multi=0, n_spliced_alns=6, n_junction_hits=10, n_long_run_alns=0)


def assert_golden(t, x):
    assert x["totals"] == GOLDEN_TOTALS
    assert len(t["gene_ids"]) == len(GOLDEN_GENES)
    for i, gid in enumerate(t["gene_ids"]):
        assert tuple(int(x["genes"][i][f]) for f in GENE_DT.names) == GOLDEN_GENES[gid], gid
    got = [(int(j["ref_id"]), int(j["start"]), int(j["end"]), "+" if j["strand"] else "-", int(j["n_unique"]), int(j["max_overhang"])) for j in x["junctions"]]
    assert got == GOLDEN_JUNCTIONS and not x["junctions"]["n_multi"].any()
    assert [sq_names(t)[k] for k in (2, 3)] == ["introns_seq", "introns_revcomp"]
    check_invariants(x)


# ------------------------------------------------------------------ SAM files
_TAG = re.compile(r"\t([A-Za-z][A-Za-z0-9]):([AiZ]):([^\t]*)")


def _sam_records(path):
    """(qname, flag, rname, pos, cigar text, tags dict) of every record line"""
    out = []
    for ln in open(path):
        if ln.startswith("@"):
            continue
        f = ln.rstrip("\n").split("\t")
        out.append((f[0], int(f[1]), f[2], int(f[3]), f[5], {k: v for k, _, v in _TAG.findall("\t" + "\t".join(f[11:]))}))
    return out


def sam_view(path, t):
    """a SAM file of the writer as (offsets, ALN_DT records, digests, words): the fields the count tables read.  The
    records of a read are consecutive; a read without alignments has the one record with flag 4."""
    recs = _sam_records(path)
    fwd_ref = {}
    for i, r in enumerate(t["refs"]):
        if r["strand"]:
            fwd_ref[t["names"][int(r["name_id"])]] = i
    offsets, alns, dig, words = [0], [], [], []
    k = 0
    while k < len(recs):
        name, flag = recs[k][0], recs[k][1]
        if flag & 4:
            offsets.append(len(alns))
            k += 1
            continue
        nh = int(recs[k][5]["NH"])
        for q, fl, rname, pos, cigar, tags in recs[k: k + nh]:
            assert q == name and int(tags["NH"]) == nh and not fl & 4
            al = np.zeros(1, capi.ALN_DT)[0]
            al["ystart"], al["ref_id"] = pos - 1, fwd_ref[rname]
            kind = tags["RE"]
            al["aln_type"] = {"E": EXONIC, "N": INTRONIC, "I": INTERGENIC}[kind]
            if kind == "E":
                al["tx_or_gene_idx"] = t["tx_ids"].index(tags["TX"].split(",")[0])
            elif kind == "N":
                al["tx_or_gene_idx"] = t["gene_ids"].index(tags["GX"])
            else:
                al["tx_or_gene_idx"] = 0xFFFFFFFF
            w = [(n << 4) | cc.BAM_CODE[c] for n, c in cc.cigar_runs(cigar)]
            d = np.zeros(1, cc.DIGEST_DT)[0]
            d["cigar_off"], d["n_cigar"] = len(words), len(w)
            d["ref_len"] = sum(n for n, c in cc.cigar_runs(cigar) if c in "MDN")
            words += w
            alns.append(al)
            dig.append(d)
        offsets.append(len(alns))
        k += nh
    return (np.array(offsets, "<u8"), np.array(alns, capi.ALN_DT) if alns else np.zeros(0, capi.ALN_DT),
            np.array(dig, cc.DIGEST_DT) if dig else np.zeros(0, cc.DIGEST_DT), np.array(words, "<u4"))


def count_sam(path, t):
    """The second way: every record line on its own.  Genes from GX + RE + NH, junctions from POS and the CIGAR text cut at
    its N runs (the anchors are the M sums of the pieces), the strand from the transcript the TX tag names.
    -> (gene rows as {gene_id: [eu, em, iu, im]}, junction rows as {(contig, start, end, '+'/'-'): [nu, nm, ov]})"""
    genes = {g: [0, 0, 0, 0] for g in t["gene_ids"]}
    rows = {}
    for q, flag, rname, pos, cigar, tags in _sam_records(path):
        if flag & 4:
            continue
        multi = int(tags["NH"]) > 1
        if tags["RE"] in "EN":
            genes[tags["GX"]][(0 if tags["RE"] == "E" else 2) + (1 if multi else 0)] += 1
        pieces = re.split(r"(\d+)N", cigar)      # piece, intron, piece, intron, ..., piece
        if len(pieces) == 1:
            continue
        strand = "+" if t["txs"][t["tx_ids"].index(tags["TX"].split(",")[0])]["strand"] else "-"
        at = pos - 1
        for k in range(1, len(pieces), 2):
            at += sum(int(n) for n, c in re.findall(r"(\d+)([MD])", pieces[k - 1]))
            ln = int(pieces[k])
            left = sum(int(n) for n in re.findall(r"(\d+)M", pieces[k - 1]))
            right = sum(int(n) for n in re.findall(r"(\d+)M", pieces[k + 1]))
            row = rows.setdefault((rname, at, at + ln, strand), [0, 0, 0])
            row[1 if multi else 0] += 1
            row[2] = max(row[2], min(left, right))
            at += ln
    return genes, rows


def tsv_of(t, x):
    """the two files of the driver for tables `x`: (genes.tsv, junctions.tsv) as text"""
    g = ["gene_id\tgene_name\texonic_unique\texonic_multi\tintronic_unique\tintronic_multi\n"]
    for i, row in enumerate(x["genes"]):
        g.append("%s\t%s\t%d\t%d\t%d\t%d\n" % ((t["gene_ids"][i], t["gene_names"][i]) + tuple(int(row[f]) for f in GENE_DT.names)))
    names = sq_names(t)
    j = ["ref\tstart\tend\tstrand\tunique\tmulti\tmax_overhang\n"]
    for row in x["junctions"]:
        j.append("%s\t%d\t%d\t%s\t%d\t%d\t%d\n" % (names[int(row["ref_id"])], int(row["start"]) + 1, int(row["end"]), "+" if row["strand"] else "-",
                                                  int(row["n_unique"]), int(row["n_multi"]), int(row["max_overhang"])))
    return "".join(g), "".join(j)


def tsv_of_sam_counts(t, genes, rows):
    """the same two files from count_sam's dictionaries"""
    g = ["gene_id\tgene_name\texonic_unique\texonic_multi\tintronic_unique\tintronic_multi\n"]
    for i, gid in enumerate(t["gene_ids"]):
        g.append("%s\t%s\t%d\t%d\t%d\t%d\n" % ((gid, t["gene_names"][i]) + tuple(genes[gid])))
    names = sq_names(t)
    j = ["ref\tstart\tend\tstrand\tunique\tmulti\tmax_overhang\n"]
    for key in sorted(rows, key=lambda k: (names.index(k[0]), k[1], k[2], k[3] == "-")):
        j.append("%s\t%d\t%d\t%s\t%d\t%d\t%d\n" % ((key[0], key[1] + 1, key[2], key[3]) + tuple(rows[key])))
    return "".join(g), "".join(j)


# ------------------------------------------------------------------ the model program's input
def model_input(t, offsets, alns, dig, words, status=None):
    """one case as the bytes tests/cpp/quant_model_main.cpp reads"""
    offsets = np.ascontiguousarray(offsets, "<u8")
    alns = np.ascontiguousarray(alns, capi.ALN_DT)
    dig = np.ascontiguousarray(dig, cc.DIGEST_DT)
    words = np.ascontiguousarray(words, "<u4")
    n_reads = len(offsets) - 1
    head = np.array([n_reads, len(alns), len(words), len(t["txs"]), len(t["genes"]), len(t["refs"]), 0 if status is None else 1], "<u8")
    parts = [head, offsets, alns, dig, words, np.ascontiguousarray(t["txs"]["gene_idx"], "<u4"),
             np.array([1 if s else 0 for s in t["txs"]["strand"]], np.uint8), np.array(ref_sq(t), "<i4")]
    if status is not None:
        parts.append(np.ascontiguousarray(status, "<i4"))
    return b"".join(p.tobytes() for p in parts)


# ------------------------------------------------------------------ views made by hand (the add_view shapes)
def make_view(reads):
    """reads: a list of reads, each a list of alignments dict(ref_id, ystart, aln_type, idx, cigar=[(len, 'M'), ...] or
    long_run=True) -> (offsets, alns, digests, words)"""
    offsets, alns, dig, words = [0], [], [], []
    for r in reads:
        for a in r:
            al = np.zeros(1, capi.ALN_DT)[0]
            al["ystart"], al["ref_id"], al["aln_type"], al["tx_or_gene_idx"] = a["ystart"], a["ref_id"], a["aln_type"], a["idx"]
            d = np.zeros(1, cc.DIGEST_DT)[0]
            d["cigar_off"] = len(words)
            if a.get("long_run"):
                d["flags"] = cc.LONG_RUN
            else:
                w = [(n << 4) | cc.BAM_CODE[c] for n, c in a["cigar"]]
                d["n_cigar"] = len(w)
                d["ref_len"] = sum(n for n, c in a["cigar"] if c in "MDN")
                words += w
            alns.append(al)
            dig.append(d)
        offsets.append(len(alns))
    return (np.array(offsets, "<u8"), np.array(alns, capi.ALN_DT) if alns else np.zeros(0, capi.ALN_DT),
            np.array(dig, cc.DIGEST_DT) if dig else np.zeros(0, cc.DIGEST_DT), np.array(words, "<u4"))


def uniform_view(n_reads, alns_per_read, ref_id, ystart, tx_idx, cigar):
    """n_reads reads of alns_per_read equal exonic alignments each, built with numpy (70 000 reads are too many for a loop
    over dictionaries)"""
    n = n_reads * alns_per_read
    w = np.array([(ln << 4) | cc.BAM_CODE[c] for ln, c in cigar], "<u4")
    alns = np.zeros(n, capi.ALN_DT)
    alns["ystart"], alns["ref_id"], alns["aln_type"], alns["tx_or_gene_idx"] = ystart, ref_id, EXONIC, tx_idx
    dig = np.zeros(n, cc.DIGEST_DT)
    dig["cigar_off"] = np.arange(n, dtype=np.uint64) * len(w)
    dig["n_cigar"] = len(w)
    dig["ref_len"] = sum(ln for ln, c in cigar if c in "MDN")
    return (np.arange(n_reads + 1, dtype="<u8") * alns_per_read, alns, dig, np.tile(w, n))


# ------------------------------------------------------------------ the shapes of thm_quant_add_view
def syn_tables():
    """the reference of the synthetic run"""
    from thermite_amd import synth
    return synth.synth_reference(length=400000, n_genes=60, seed=7)


def syn_reads(t):
    from thermite_amd import synth
    bases, off, _ = synth.simulate_reads(t, 4000, 91)
    return bases, off


def big_gene_tables(n_genes=12000):
    """12 000 single-exon genes of 100 bases on a random contig of 1.3 M bases: 48 000 gene counters"""
    from thermite_amd import refdata
    rng = np.random.default_rng(12000)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 1300000)]
    genes = [dict(id="BIGG%05d" % g, name="big%d" % g) for g in range(n_genes)]
    txs = [dict(id="BIGT%05d" % g, gene_idx=g, chrom="bigsyn", strand=bool(g % 3), exons=[(500 + 105 * g, 600 + 105 * g)]) for g in range(n_genes)]
    return refdata.build_tables([("bigsyn", seq)], genes, txs)


def _tx_of_strand(t, forward):
    return int(np.nonzero(t["txs"]["strand"] == (1 if forward else 0))[0][0])


def shape_cases(t):
    """name -> list of views (each added in turn) over the tables `t` of syn_tables()"""
    fwd, rev = _tx_of_strand(t, True), _tx_of_strand(t, False)
    spliced = [(30, "M"), (500, "N"), (61, "M")]
    many = [(3, "S"), (7, "M")]
    for k in range(40):
        many += [(100 + k, "N")]
        if k == 17:
            many += [(90, "N")]                    # two adjacent N words: anchor 0 between them
        many += [(2, "M"), (1, "I"), (1 + k % 3, "M"), (2, "D"), (k % 5, "M")] if k % 2 else [(4 + k, "M")]
    many += [(2, "S")]
    exon = dict(ref_id=0, aln_type=EXONIC)
    return {
        "empty": [make_view([])],
        "no_alignments": [make_view([[], [], []])],
        "one_read_5000": [uniform_view(1, 5000, 0, 1000, fwd, spliced)],
        "unique_70000": [uniform_view(70000, 1, 0, 2000, rev, spliced)],
        "forty_introns": [make_view([[dict(exon, ystart=5000, idx=fwd, cigar=many)], [],
                                     [dict(exon, ystart=5000, idx=fwd, cigar=many), dict(exon, ystart=5010, idx=rev, cigar=many[1:])]])],
        "long_run": [make_view([[dict(exon, ystart=100, idx=fwd, long_run=True)], [dict(exon, ystart=100, idx=fwd, cigar=spliced)]])],
        "both_strands": [make_view([[dict(exon, ystart=7000, idx=fwd, cigar=spliced)], [dict(exon, ystart=7000, idx=rev, cigar=spliced)],
                                    [dict(ref_id=1, ystart=7000, aln_type=EXONIC, idx=rev, cigar=spliced)]])],
        "later_overhang": [make_view([[dict(exon, ystart=9000, idx=fwd, cigar=[(5, "M"), (300, "N"), (86, "M")])]]),
                           make_view([[dict(exon, ystart=8990, idx=fwd, cigar=[(15, "M"), (300, "N"), (40, "M"), (2, "I"), (34, "M")])],
                                      [dict(ref_id=0, ystart=1, aln_type=INTRONIC, idx=3, cigar=[(91, "M")]),
                                       dict(ref_id=1, ystart=50, aln_type=INTERGENIC, idx=0xFFFFFFFF, cigar=[(91, "M")])]]),
                           make_view([[dict(exon, ystart=8998, idx=fwd, cigar=[(7, "M"), (300, "N"), (84, "M")])]])],
    }


def big_gene_view(t, n_random=20000):
    """one exonic alignment on every gene of big_gene_tables() plus n_random at random, a third of them spliced"""
    rng = np.random.default_rng(7)
    n = len(t["genes"])
    tx = np.concatenate([np.arange(n), rng.integers(0, n, n_random)])
    rng.shuffle(tx)
    alns = np.zeros(len(tx), capi.ALN_DT)
    alns["aln_type"], alns["tx_or_gene_idx"], alns["ystart"] = EXONIC, tx, 500 + 105 * tx
    alns["ref_id"] = np.where(t["txs"]["strand"][tx] != 0, 0, 1)
    kinds = [np.array([(50 << 4) | M], "<u4"), np.array([(20 << 4) | M, (200 << 4) | N, (30 << 4) | M], "<u4")]
    which = (np.arange(len(tx)) % 3 == 0).astype(int)
    dig = np.zeros(len(tx), cc.DIGEST_DT)
    lens = np.where(which == 1, 3, 1)
    dig["n_cigar"] = lens
    dig["cigar_off"] = np.cumsum(lens) - lens
    dig["ref_len"] = np.where(which == 1, 250, 50)
    words = np.concatenate([kinds[k] for k in which])
    # reads of one, two and three alignments
    cuts, at = [0], 0
    while at < len(tx):
        at = min(at + 1 + int(rng.integers(0, 3)), len(tx))
        cuts.append(at)
    return np.array(cuts, "<u8"), alns, dig, words
