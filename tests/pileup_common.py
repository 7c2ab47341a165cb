"""What the per-base allele counts of a run must hold (include/thermite_io.h, above thm_pileup_create), written from that
contract alone: `Expect` walks a view (offsets, records, digests, words -- the tuples of quant_common.py -- plus the reads'
bytes) into dense per-contig arrays of seven counters with np.add.at and cuts rows out of them; `sam_pileup` counts a SAM
file and the FASTA a second, independent way -- line by line from POS, the CIGAR text, SEQ, the flag and NH, a base at a
time into dictionaries.  Nothing here touches the library under test."""
import re

import numpy as np

import cigar_common as cc
import cov_common as cv
import quant_common as qc
from thermite_amd import capi

MULTI = 1
SITE_DT = np.dtype([("ref_id", "<u4"), ("ref_base", "u1"), ("pad_", "u1", (3,)), ("pos", "<u8"), ("depth", "<u4"), ("cnt", "<u4", (5,)),
                    ("del", "<u4"), ("ins", "<u4")])
TOTAL_NAMES = ["n_reads", "n_failed_reads", "n_alns", "n_skipped_multi", "n_long_run_alns", "n_used_alns", "n_blocks", "n_m_bases",
               "n_mismatches", "n_del_bases", "n_ins", "n_ins_bases"]
M, I, D, N, S = 0, 1, 2, 3, 4
K_N, K_DEL, K_INS = 4, 5, 6
TSV_HEADER = "#contig\tpos\tref\tdepth\tA\tC\tG\tT\tN\tdel\tins\n"

KIND = np.full(256, K_N, np.uint8)            # kind(c) of the contract
for _k, _c in enumerate(b"ACGT"):
    KIND[_c] = KIND[_c + 32] = _k
COMP_KIND = np.array([3, 2, 1, 0, 4], np.uint8)


def seq_kinds(read, forward):
    """the kinds of SEQ: the read's, or those of its reverse complement"""
    read = np.asarray(read, np.uint8)
    return KIND[read] if forward else COMP_KIND[KIND[read[::-1]]]


def contig_seqs(t):
    """the sequence of every @SQ contig: the forward copy in the text"""
    sq, out = qc.ref_sq(t), {}
    for i, r in enumerate(t["refs"]):
        if r["strand"]:
            out[sq[i]] = np.asarray(t["text"][int(r["start_idx"]): int(r["start_idx"]) + int(r["len"])], np.uint8)
    return [out[s] for s in range(len(out))]


class Expect:
    """the counts of an object created with `flags` over the tables `t`, and its totals"""

    def __init__(self, t, flags):
        self.t, self.flags, self.sq, self.seqs = t, flags, qc.ref_sq(t), contig_seqs(t)
        self.lens = [len(s) for s in self.seqs]
        assert self.lens == cv.sq_lengths(t)
        self.cnt = [np.zeros((n, 7), np.int64) for n in self.lens]
        self.diff = [np.zeros(n + 1, np.int64) for n in self.lens]
        self.totals = dict.fromkeys(TOTAL_NAMES, 0)

    def add(self, offsets, alns, dig, words, bases, base_off, status=None):
        """-> the batch's totals"""
        tot = dict.fromkeys(TOTAL_NAMES, 0)
        offsets = [int(x) for x in offsets]
        base_off = [int(x) for x in base_off]
        bases = np.asarray(bases, np.uint8)
        n_reads = max(len(offsets) - 1, 0)
        tot["n_reads"] = n_reads
        if status is not None:
            tot["n_failed_reads"] = int((np.asarray(status) != 0).sum())
        obs = [([], []) for _ in self.lens]        # (positions, kinds) per contig
        ends = [([], []) for _ in self.lens]
        words = np.asarray(words)
        for r in range(n_reads):
            multi = offsets[r + 1] - offsets[r] > 1
            read = bases[base_off[r]: base_off[r + 1]]
            for a in range(offsets[r], offsets[r + 1]):
                al, d = alns[a], dig[a]
                tot["n_alns"] += 1
                if multi and not self.flags & MULTI:
                    tot["n_skipped_multi"] += 1
                    continue
                if int(d["flags"]) & cc.LONG_RUN:
                    tot["n_long_run_alns"] += 1
                    continue
                tot["n_used_alns"] += 1
                o, s, ystart = int(d["cigar_off"]), self.sq[int(al["ref_id"])], int(al["ystart"])
                w = [(int(x) >> 4, int(x) & 15) for x in words[o: o + int(d["n_cigar"])]]
                if not w:
                    continue
                assert sum(n for n, c in w if c in (M, I, S)) == len(read), "M + I + S is not the read's length"
                if not sum(n for n, c in w if c in (M, D, N)):
                    continue
                kinds = seq_kinds(read, int(al["strand"]) == 1)
                p, q = ystart, 0
                for n, c in w:
                    if c == M:
                        obs[s][0].append(np.arange(p, p + n))
                        obs[s][1].append(kinds[q: q + n])
                        tot["n_m_bases"] += n
                        tot["n_mismatches"] += int((kinds[q: q + n] != KIND[self.seqs[s][p: p + n]]).sum())
                        p, q = p + n, q + n
                    elif c == D:
                        obs[s][0].append(np.arange(p, p + n))
                        obs[s][1].append(np.full(n, K_DEL, np.uint8))
                        tot["n_del_bases"] += n
                        p += n
                    elif c == N:
                        p += n
                    elif c == I:
                        obs[s][0].append(np.array([p - 1 if p > ystart else ystart]))
                        obs[s][1].append(np.array([K_INS], np.uint8))
                        tot["n_ins"] += 1
                        tot["n_ins_bases"] += n
                        q += n
                    elif c == S:
                        q += n
                blocks = cv.blocks_of(words[o: o + int(d["n_cigar"])], ystart)
                tot["n_blocks"] += len(blocks)
                for b, e in blocks:
                    assert e <= self.lens[s], "a block beyond its contig"
                    ends[s][0].append(b)
                    ends[s][1].append(e)
        for s in range(len(self.lens)):
            if obs[s][0]:
                np.add.at(self.cnt[s], (np.concatenate(obs[s][0]), np.concatenate(obs[s][1]).astype(np.int64)), 1)
            np.add.at(self.diff[s], np.array(ends[s][0], np.int64), 1)
            np.add.at(self.diff[s], np.array(ends[s][1], np.int64), -1)
        for f in TOTAL_NAMES:
            self.totals[f] += tot[f]
        return tot

    def depth(self, s):
        d = np.cumsum(self.diff[s])
        assert d[-1] == 0 and d.min() >= 0
        return d[:-1]

    def events(self, s):
        """cnt with the reference allele's column zeroed: what the table holds"""
        ev = self.cnt[s].copy()
        ev[np.arange(self.lens[s]), KIND[self.seqs[s]]] = 0
        return ev

    def alt(self, s):
        return self.events(s).sum(axis=1)

    def n_events(self, first_ref=0, n_refs=None):
        n_refs = len(self.lens) - first_ref if n_refs is None else n_refs
        return sum(int((self.events(s) != 0).sum()) for s in range(first_ref, first_ref + n_refs))

    def _rows(self, s, pos):
        out = np.zeros(len(pos), SITE_DT)
        out["ref_id"], out["pos"], out["ref_base"], out["depth"] = s, pos, self.seqs[s][pos], self.depth(s)[pos]
        out["cnt"], out["del"], out["ins"] = self.cnt[s][pos, :5], self.cnt[s][pos, K_DEL], self.cnt[s][pos, K_INS]
        assert (out["depth"] == out["cnt"].sum(axis=1) + out["del"]).all(), "depth == sum(cnt) + del"
        return out

    def rows(self, first_ref=0, n_refs=None, min_alt=1):
        n_refs = len(self.lens) - first_ref if n_refs is None else n_refs
        parts = [self._rows(s, np.flatnonzero(self.alt(s) >= min_alt)) for s in range(first_ref, first_ref + n_refs)]
        return np.concatenate(parts) if parts else np.zeros(0, SITE_DT)

    def window(self, s, start, n):
        return self._rows(s, np.arange(start, start + n))

    def scaled(self, k):
        out = Expect(self.t, self.flags)
        out.cnt, out.diff = [c * k for c in self.cnt], [d * k for d in self.diff]
        out.totals = {f: v * k for f, v in self.totals.items()}
        return out


def from_oracle(t, flags, result, bases, off, status=None):
    dig, words = cc.expected_alignments(result.alns, result.ops)
    e = Expect(t, flags)
    e.add(result.offsets, result.alns, dig, words, bases, off, status)
    return e


def assert_sites_equal(got, exp, what=""):
    assert len(got) == len(exp), (what, len(got), len(exp), got[:5], exp[:5])
    for f in SITE_DT.names if len(got) else ():
        bad = np.nonzero((got[f] != exp[f]).reshape(len(got), -1).any(axis=1))[0]
        assert len(bad) == 0, "%s site %d %s: got %s expected %s" % (what, bad[0], f, got[bad[0]], exp[bad[0]])
    assert np.ascontiguousarray(got, SITE_DT).tobytes() == np.ascontiguousarray(exp, SITE_DT).tobytes(), what


def check_fetch(res, exp, first_ref=0, n_refs=None, min_alt=1, what=""):
    """a capi.PileupResult of a fetch against the expectation"""
    assert_sites_equal(res.sites, exp.rows(first_ref, n_refs, min_alt), "%s min_alt %d" % (what, min_alt))
    assert res.n_events == exp.n_events(first_ref, n_refs), (what, res.n_events, exp.n_events(first_ref, n_refs))
    assert res.totals == exp.totals, (what, res.totals, exp.totals)
    assert res.min_alt == min_alt


def check_window(res, exp, s, start, n, what=""):
    assert_sites_equal(res.sites, exp.window(s, start, n), "%s window %d %d +%d" % (what, s, start, n))
    assert res.n_events == int((exp.events(s)[start: start + n] != 0).sum()), what
    assert (res.sites["depth"] == res.sites["cnt"].sum(axis=1) + res.sites["del"]).all(), what


def check_invariants(exp):
    tot = exp.totals
    assert tot["n_alns"] == tot["n_skipped_multi"] + tot["n_long_run_alns"] + tot["n_used_alns"]
    ev = sum(int(exp.events(s).sum()) for s in range(len(exp.lens)))
    assert ev == tot["n_mismatches"] + tot["n_del_bases"] + tot["n_ins"]
    assert sum(int(exp.cnt[s][:, :5].sum()) for s in range(len(exp.lens))) == tot["n_m_bases"]
    for s in range(len(exp.lens)):
        assert (exp.depth(s) == exp.cnt[s][:, :6].sum(axis=1)).all()


def tsv(names, rows):
    """the driver's <output>.pileup.tsv for SITE_DT rows"""
    out = [TSV_HEADER]
    for r in rows:
        out.append("%s\t%d\t%s\t%d\t%s\t%d\t%d\n" % (names[int(r["ref_id"])], int(r["pos"]) + 1, chr(int(r["ref_base"])), int(r["depth"]),
                                                     "\t".join(str(int(x)) for x in r["cnt"]), int(r["del"]), int(r["ins"])))
    return "".join(out)


# ------------------------------------------------------------------ SAM files
def sam_view(path, t):
    """cov_common.sam_view, and the reads' bytes from SEQ: (offsets, alns, digests, words, bases, base_off)"""
    off, alns, dig, words = cv.sam_view(path, t)
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    reads, k = [], 0
    lines = [ln.rstrip("\n").split("\t") for ln in open(path) if not ln.startswith("@")]
    while k < len(lines):
        f = lines[k]
        flag, seq = int(f[1]), f[9].encode()
        reads.append(seq.translate(comp)[::-1] if flag & 0x10 else seq)
        k += 1 if flag & 4 else int(re.search(r"\tNH:i:(\d+)", "\t".join(f)).group(1))
    assert len(reads) == len(off) - 1
    base_off = np.cumsum([0] + [len(r) for r in reads]).astype("<u8")
    return off, alns, dig, words, np.frombuffer(b"".join(reads), np.uint8), base_off


def parse_fasta_text(path):
    """[(name, upper-cased sequence as str)] of a FASTA file"""
    out = []
    for ln in open(path):
        ln = ln.strip()
        if ln.startswith(">"):
            out.append([ln[1:].split(" ")[0], []])
        elif ln:
            out[-1][1].append(ln.upper())
    return [(n, "".join(s)) for n, s in out]


def sam_pileup(sam_path, fasta, names, multi=False, min_alt=1):
    """The second way: every record line on its own, a base at a time -- POS, the CIGAR text, SEQ as printed, flag 4 and the
    NH tag against the FASTA's sequences (`fasta`: [(name, str)]).  `names`: the contigs in @SQ order.
    -> [(contig, 0-based pos, ref, depth, A, C, G, T, N, del, ins)] of the sites with min_alt events or more"""
    ref = dict(fasta)
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    cnt, depth = {}, {}
    for ln in open(sam_path):
        if ln.startswith("@"):
            continue
        f = ln.rstrip("\n").split("\t")
        if int(f[1]) & 4:
            continue
        nh = int(re.search(r"\tNH:i:(\d+)", ln).group(1))
        if nh > 1 and not multi:
            continue
        rname, ystart, seq = f[2], int(f[3]) - 1, f[9].upper()
        ops = [(int(n), c) for n, c in re.findall(r"(\d+)([MIDNS])", f[5])]
        assert sum(n for n, c in ops if c in "MIS") == len(seq)
        if not any(c in "MDN" and n for n, c in ops):
            continue
        p, q = ystart, 0
        for n, c in ops:
            if c == "M":
                for i in range(n):
                    cnt.setdefault((rname, p + i), [0] * 7)[code.get(seq[q + i], 4)] += 1
                    depth[(rname, p + i)] = depth.get((rname, p + i), 0) + 1
                p, q = p + n, q + n
            elif c == "D":
                for i in range(n):
                    cnt.setdefault((rname, p + i), [0] * 7)[K_DEL] += 1
                    depth[(rname, p + i)] = depth.get((rname, p + i), 0) + 1
                p += n
            elif c == "N":
                p += n
            elif c == "I":
                cnt.setdefault((rname, p - 1 if p > ystart else ystart), [0] * 7)[K_INS] += 1
                q += n
            else:
                q += n
    out = []
    for (rname, x), c in cnt.items():
        rb = ref[rname][x]
        alt = sum(c) - (c[code.get(rb, 4)])
        if alt >= min_alt:
            out.append((rname, x, rb, depth.get((rname, x), 0)) + tuple(c))
    return sorted(out, key=lambda r: (names.index(r[0]), r[1]))


def tsv_of_sam(rows):
    return TSV_HEADER + "".join("%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % ((r[0], r[1] + 1) + r[2:]) for r in rows)


def rows_as_tuples(names, rows):
    return [(names[int(r["ref_id"])], int(r["pos"]), chr(int(r["ref_base"])), int(r["depth"])) + tuple(int(x) for x in r["cnt"]) +
            (int(r["del"]), int(r["ins"])) for r in rows]


# ------------------------------------------------------------------ the model program's input
def model_input(t, flags, views, windows=()):
    """what tests/cpp/pileup_model_main.cpp reads: the layout and the text, the windows (refID, start, n) and the views,
    each added in turn"""
    sq, seqs = qc.ref_sq(t), contig_seqs(t)
    text = np.concatenate([np.concatenate([s, np.frombuffer(b"$", np.uint8)]) for s in seqs])
    tstart = np.cumsum([0] + [len(s) + 1 for s in seqs])[:-1]
    parts = [np.array([flags, len(sq), len(seqs), len(windows), len(views), len(text)], "<u8"), np.array(sq, "<i4"),
             np.array([len(s) for s in seqs], "<u8"), np.array(tstart, "<u8"), text, np.array(list(windows), "<u8").reshape(-1)]
    for offsets, alns, dig, words, bases, base_off, *rest in views:
        status = rest[0] if rest else None
        offsets, base_off = np.ascontiguousarray(offsets, "<u8"), np.ascontiguousarray(base_off, "<u8")
        if len(offsets) == 0:
            offsets = base_off = np.zeros(1, "<u8")
        parts += [np.array([len(offsets) - 1, len(alns), len(words), 0 if status is None else 1, len(bases)], "<u8"), offsets,
                  np.ascontiguousarray(alns, capi.ALN_DT), np.ascontiguousarray(dig, cc.DIGEST_DT), np.ascontiguousarray(words, "<u4"),
                  base_off, np.ascontiguousarray(bases, np.uint8)]
        if status is not None:
            parts.append(np.ascontiguousarray(status, "<i4"))
    return b"".join(p.tobytes() for p in parts)


def model_output(windows, out):
    """-> (totals dict, n_events, [rows at min_alt 1, 2, 3], [rows per window])"""
    tot = {k: int(v) for k, v in zip(TOTAL_NAMES, np.frombuffer(out[:96], "<u8"))}
    n_events = int(np.frombuffer(out[96:104], "<u8")[0])
    at, fetches, wins = 104, [], []
    for _ in range(3):
        n = int(np.frombuffer(out[at: at + 8], "<u8")[0])
        fetches.append(np.frombuffer(out[at + 8: at + 8 + 48 * n], SITE_DT))
        at += 8 + 48 * n
    for _, _, n in windows:
        wins.append(np.frombuffer(out[at: at + 48 * n], SITE_DT))
        at += 48 * n
    assert at == len(out)
    return tot, n_events, fetches, wins


# ------------------------------------------------------------------ views made by hand (the add_view shapes)
CONTIG = 20000
N_AT = (300, 301, 7000)          # N bases of the first contig's reference


def shape_tables():
    """three contigs made for the shapes: two of 20 000 bases (five tiles of the fetch) and one of 1000 between them; the
    first has N bases at N_AT"""
    from thermite_amd import refdata
    rng = np.random.default_rng(419)
    seq = lambda n: np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    a = seq(CONTIG)
    a[list(N_AT)] = ord("N")
    genes = [dict(id="PILG%d" % g, name="pile%d" % g) for g in range(2)]
    txs = [dict(id="PILT0", gene_idx=0, chrom="pile_a", strand=True, exons=[(1000, 1400), (2000, 2300)]),
           dict(id="PILT1", gene_idx=1, chrom="pile_b", strand=False, exons=[(5000, 5600)])]
    return refdata.build_tables([("pile_a", a), ("pile_small", seq(1000)), ("pile_b", seq(CONTIG))], genes, txs)


_OTHER = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A"), ord("N"): ord("A")}
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


class Shapes:
    """builds views over shape_tables(): an alignment is dict(s=@SQ entry, at=ystart, cigar=[(len, 'M'), ...], strand=1,
    edits={SEQ index: byte or None for 'another base'}); its read's bytes follow the reference through the CIGAR, with the
    inserted and clipped bases drawn at random, the edits applied to SEQ, and the whole reverse-complemented for strand 0"""

    def __init__(self, t):
        self.t, self.seqs, self.rng = t, contig_seqs(t), np.random.default_rng(7)

    def seq_of(self, al):
        out, p = [], al["at"]
        for n, c in al["cigar"]:
            if c == "M":
                out.append(self.seqs[al["s"]][p: p + n])
            elif c in "IS":
                out.append(np.frombuffer(b"ACGT", np.uint8)[self.rng.integers(0, 4, n)])
            if c in "MDN":
                p += n
        seq = np.concatenate(out).copy() if out else np.zeros(0, np.uint8)
        for i, b in al.get("edits", {}).items():
            seq[i] = _OTHER[int(seq[i])] if b is None else b
        return seq

    def view(self, reads):
        """reads: a list of reads, each a list of alignments (the read's bytes come from its first, or from SEQ given as `seq=` there)"""
        flat, bases = [], []
        for r in reads:
            seq = np.zeros(0, np.uint8)
            if r:
                seq = np.asarray(r[0]["seq"], np.uint8) if "seq" in r[0] else self.seq_of(r[0])
                if r[0].get("strand", 1) != 1:
                    seq = np.frombuffer(bytes(seq).translate(_COMP)[::-1], np.uint8)
            bases.append(seq)
            flat.append([dict(ref_id=cv.ref_of(self.t, a["s"], a.get("strand", 1) == 1), ystart=a["at"], strand=a.get("strand", 1), cigar=a["cigar"]) for a in r])
        off, alns, dig, words = cv.make_view(flat)
        base_off = np.cumsum([0] + [len(b) for b in bases]).astype("<u8")
        return off, alns, dig, words, (np.concatenate(bases) if bases else np.zeros(0, np.uint8)), base_off


def shape_cases(t, chunk, group, tile):
    """name -> list of views (each added in turn) over shape_tables()"""
    sh = Shapes(t)
    one = lambda s, at, cigar, **kw: [dict(s=s, at=at, cigar=cigar, **kw)]
    ends = lambda n: {0: None, n - 1: None}
    assert contig_lens(t) == [CONTIG, 1000, CONTIG] and tile * 4 < CONTIG
    lengths = sorted({1, chunk - 1, chunk, chunk + 1, group * chunk - 1, group * chunk + 1, 5000})
    # both sides of every chunk edge, counted from the front and -- for the reads taken from their end -- from the back
    edge_edits = lambda n: {j: None for k in range(0, n + chunk, chunk) for i in (k - 1, k) if 0 <= i < n for j in (i, n - 1 - i)}
    many = [(3, "S"), (7, "M")]
    for k in range(40):
        many += [(100 + k, "N")] + ([(2, "M"), (1, "I"), (1 + k % 3, "M"), (2, "D"), (1 + k % 5, "M")] if k % 2 else [(4 + k, "M")])
    n_many = sum(n for n, c in many if c in "MIS")
    next_to = {}
    for op in "SIDN":
        first = [(4, "M"), (2, op), (6, "M")] if op in "IDN" else [(2, "S"), (10, "M")]
        last = first if op in "IDN" else [(10, "M"), (2, "S")]
        # the last base of the M word in front of the op and the first base of the one behind it (SEQ indices)
        e1 = {3: None, 4 + (2 if op == "I" else 0): None} if op in "IDN" else {2: None}
        e2 = e1 if op in "IDN" else {9: None}
        next_to[op] = [sh.view([one(0, 500, first, edits=e1), one(2, 800, last, edits=e2, strand=0 if op == "S" else 1)])]
    hot_al = dict(s=2, at=12345, cigar=[(50, "M")], edits={17: ord("A") if sh.seqs[2][12362] != ord("A") else ord("C")})
    hot = sh.view([[hot_al]])
    n = 5000
    hot_many = (np.arange(n + 1, dtype="<u8"), np.repeat(hot[1], n), np.repeat(hot[2], n), hot[3], np.tile(hot[4], n), np.arange(n + 1, dtype="<u8") * 50)
    x = 9000                                       # one position that sees everything; behind it sites with 1, 2 and 3 events
    every = [one(0, x - 5, [(11, "M")], edits={5: b}) for b in b"ACGTN"] + [one(0, x - 5, [(5, "M"), (1, "D"), (5, "M")]),
                                                                            one(0, x - 5, [(6, "M"), (3, "I"), (5, "M")])]
    t_edge = [one(0, tile - 6, [(12, "M")], edits={5: None, 6: None}), one(0, 3 * tile + 100, [(9, "M")], edits={4: None}),
              one(2, 2 * tile - 1, [(1, "M")], edits={0: None}), one(2, 2 * tile, [(1, "M")], edits={0: None})]
    return dict({
        "empty": [sh.view([])],
        "no_alignments": [sh.view([[], [], []])],
        "perfect": [sh.view([one(0, 1000, [(91, "M")]), one(2, 40, [(30, "M"), (500, "N"), (61, "M")], strand=0)])],
        "contig_ends": [sh.view([one(1, 0, [(40, "M")], edits={0: None}), one(1, 960, [(40, "M")], edits={39: None}),
                                 one(2, CONTIG - 10, [(10, "M")], edits={9: None}, strand=0)])],
        "ins_behind_s_and_n": [sh.view([one(0, 600, [(3, "S"), (2, "I"), (8, "M")]), one(0, 700, [(5, "M"), (20, "N"), (2, "I"), (5, "M")]),
                                        one(0, 900, [(2, "I"), (1, "M"), (3, "I"), (6, "M")])])],
        "d_next_to_n": [sh.view([one(0, 1500, [(5, "M"), (2, "D"), (30, "N"), (3, "D"), (5, "M")])])],
        "reverse_ends": [sh.view([one(0, 2500, [(91, "M")], edits=ends(91), strand=0), one(2, 2500, [(3, "S"), (40, "M"), (2, "S")], edits={3: None, 42: None}, strand=0)])],
        "lengths": [sh.view([one(k % 2 * 2, 3000 + 13 * k, [(n, "M")], edits=edge_edits(n), strand=k % 2) for k, n in enumerate(lengths)] +
                            [one(0, 4000, [(n, "M")], edits=edge_edits(n), strand=0) for n in lengths[:-1]])],
        "forty_introns": [sh.view([one(0, 5000, many, edits={3: None, n_many - 1: None}), [], one(0, 5000, many, strand=0)])],
        "hot_same_mismatch": [hot_many],
        "hot_every_kind": [sh.view(every + every[:3] + [one(0, x - 5, [(11, "M")], edits={5 + k: None}) for k in (1, 2, 3) for _ in range(k)])],
        "tile_edges": [sh.view(t_edge)],
        "letters": [sh.view([[dict(s=0, at=1000, cigar=[(12, "M")], seq=np.frombuffer(bytes(sh.seqs[0][1000:1012]).lower(), np.uint8))],
                             one(0, 1100, [(10, "M")], edits={2: ord("N"), 5: ord("n"), 7: ord("R"), 8: ord("*")}),
                             one(0, 295, [(10, "M")], edits={5: ord("N"), 6: ord("A")}),                # N under N: no event; A under N: one
                             one(0, 6995, [(10, "M")], edits={5: ord("n")}, strand=0)])],
        "long_run": [long_run_case(t)],
        "multi": [sh.view([one(0, 200, [(50, "M")], edits={7: None}) + one(2, 300, [(50, "M")]), one(0, 220, [(50, "M")], edits={9: None})])],
        "later_add": [sh.view([one(0, 9000, [(100, "M")], edits={10: None, 50: None}), one(2, 50, [(91, "M")], edits={0: None})]),
                      sh.view([one(0, 9040, [(20, "M")], edits={10: None}), one(0, 9100, [(10, "M")], edits={3: None})]),
                      sh.view([one(0, 8990, [(10, "M"), (2, "D"), (8, "M"), (3, "I"), (30, "M")], edits={0: None})])],
    }, **{"next_to_" + op: v for op, v in next_to.items()})


def long_run_case(t):
    """the long_run shape's second alignment with the long-run digest in place of its words"""
    sh = Shapes(t)
    off, alns, dig, words, bases, base_off = sh.view([[dict(s=0, at=100, cigar=[(30, "M")], edits={3: None})],
                                                      [dict(s=0, at=100, cigar=[(30, "M"), (500, "N"), (61, "M")])]])
    dig = dig.copy()
    dig["flags"][1] = cc.LONG_RUN
    dig["n_cigar"][1] = 0
    return off, alns, dig, words, bases, base_off


def contig_lens(t):
    return cv.sq_lengths(t)


def shape_windows(tile):
    """(refID, start, n) windows of thm_pileup_window for the shapes"""
    return [(0, 0, 1), (0, 8990, 200), (0, tile - 3, 2 * tile + 7), (0, CONTIG - 40, 40), (1, 0, 1000), (1, 999, 1), (2, 12300, 200), (2, 2 * tile - 2, 4), (0, 280, 40)]


def bad_views(t):
    """name -> a view that must be refused, naming alignment 1"""
    sh = Shapes(t)
    good = [dict(s=0, at=100, cigar=[(50, "M")])]
    past = sh.view([good, [dict(s=1, at=950, cigar=[(20, "M"), (10, "N"), (21, "M")], seq=np.full(41, ord("A"), np.uint8))]])   # ends at 1001 of 1000
    short = list(sh.view([good, good]))
    short[5] = short[5].copy()
    short[5][2] -= 1                                                     # the second read loses a base
    short[4] = short[4][:-1]
    return {"past_the_contig": past, "query_length": tuple(short)}
