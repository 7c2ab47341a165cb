"""Shared by tests/test_contigs_host.py, tests/test_gpu_contigs.py and bam_common.py: a reference of many contigs -- a few
large ones, dozens shorter than a kilobase, a run of fourteen of at most 80 bases, contigs of 1, 2, k - 1 and k bases --
whose names are not in byte order, with paralogous segments and repeat families spread over the contigs, N runs at contig
ends, genes flush with contig ends, and the reads that reach what only such a reference has: contig-copy boundaries inside
one 1024-symbol bin (idx_to_ref), alignments that overlap in [ystart, yend) on different contigs (filter_overlapping and
its name_rank), windows clamped at both ends of short contigs.  Everything comes from seeded generators and is made once
per process."""
import numpy as np

import smem_finish_common as sf
from gpu_common import mutate
from thermite_amd import capi, refdata, synth

_ACGT = np.frombuffer(b"ACGT", np.uint8)
L0 = 91
K = capi.CI_OPTS["min_seed_len"]
SEED = 0x636F6E74696773
GRID_SHIFT = 10            # thermite_internal.h
KEYCAP = 16                # extend_plan.h
P1_AT, P1_LEN = 2000, 1300
FAM_LEN, FAM_SLOT = 120, 130
F2_COPIES, F4_COPIES = 24, 12
F3_DIVERGENCE = 0.015
TAIL_FREE = 600            # the last bases of a large contig: no planted copy (an edge gene or a telomere)
TINY_OPTS = dict(capi.CI_OPTS, min_aln_score=0)   # for the contigs an alignment of 30 bases does not fit into
WIDE_OPTS = dict(capi.CI_OPTS, min_aln_score_percent=0.5)   # 300 bases: band +-150, beyond four cells per lane

LARGE = [("chr2", 36000), ("chr10", 32000), ("chr1", 28000), ("MT", 24000), ("chrX", 20000), ("chr3", 16000)]
MEDIUM = [("KI270_b", 5000), ("KI270_a", 3000), ("chrUn_9", 2000), ("chrUn_10", 1200), ("GL_3", 800), ("GL_12", 400)]
SCAF_FIXED = {0: 90, 1: 91, 2: 92, 3: 300, 4: 70, 5: 64, 6: 1500, 7: 30, 8: 1023, 9: 1024, 10: 1025, 11: 200, 12: 150, 13: 100}
N_SCAF, N_TINY = 45, 14
SMALLEST = [1, 2, K - 1, K]
SCAF_WHOLE_91, SCAF_GENE_300, SCAF_SHORT_TX, SCAF_ALL_N = "scaf1", "scaf3", "scaf4", "scaf5"

_memo = {}


def _rand(rng, n):
    return _ACGT[rng.integers(0, 4, n)].copy()


def _substitute(rng, a, rate):
    a = a.copy()
    for p in np.nonzero(rng.random(len(a)) < rate)[0]:
        a[p] = sf.substitute(a, int(p), rng)[p]
    return a


def _file_order(rng):
    """(name, length, kind) in file order: the large contigs apart from each other, the short ones between them"""
    scaf = [("scaf%d" % i, SCAF_FIXED.get(i) or int(rng.integers(30, 901)), "scaf") for i in range(N_SCAF)]
    tiny = [("tiny%d" % i, int(rng.integers(30, 81)), "tiny") for i in range(N_TINY)]
    small = [("z%d" % n, n, "small") for n in SMALLEST]
    lg = [(n, l, "large") for n, l in LARGE]
    md = [(n, l, "medium") for n, l in MEDIUM]
    return ([lg[0]] + scaf[0:5] + [lg[1]] + md[0:2] + scaf[5:15] + [lg[2]] + tiny + [lg[3]] + md[2:4] + scaf[15:30] + small +
            [lg[4]] + md[4:6] + scaf[30:45] + [lg[5]])


def _make():
    rng = np.random.Generator(np.random.PCG64([SEED, 1]))
    order = _file_order(rng)
    seqs = {name: _rand(rng, n) for name, n, _ in order}
    seqs[SCAF_ALL_N][:] = ord("N")
    p1 = _rand(rng, P1_LEN)
    fam = {k: _rand(rng, FAM_LEN) for k in ("F2", "F3", "F4")}
    whole91 = seqs[SCAF_WHOLE_91]
    plants = {"F2": [], "F3": [], "F4": [], "whole91": []}    # (contig, start, forward)
    gene_end = {}
    for li, (name, n) in enumerate(LARGE):
        s = seqs[name]
        region = int(0.35 * n)
        g_end = n - TAIL_FREE - region
        gene_end[name] = g_end
        kinds = ["F2"] * (F2_COPIES // len(LARGE)) + ["F4"] * (F4_COPIES // len(LARGE)) + (["whole91"] if li == 0 else [])
        n_slots = region // FAM_SLOT
        kinds += ["F3"] * (n_slots - len(kinds))
        for j, i in enumerate(rng.permutation(n_slots)):
            kind, at = kinds[i], g_end + j * FAM_SLOT
            forward = bool((i + li) & 1) if kind != "F3" else bool(rng.random() < 0.5)
            unit = whole91 if kind == "whole91" else fam[kind]
            if kind == "F3":
                unit = _substitute(rng, unit, F3_DIVERGENCE)
            s[at: at + len(unit)] = unit if forward else refdata.revcomp(unit)
            plants[kind].append((name, at, forward))
    for li, (name, n) in enumerate(LARGE):   # paralog segment: exact on three, reverse-complemented on one, 2 % off on two
        unit = p1 if li < 3 else refdata.revcomp(p1) if li == 3 else _substitute(rng, p1, 0.02)
        seqs[name][P1_AT: P1_AT + P1_LEN] = unit
    n_runs = {"chr10": (0, 500), "MT": (24000 - 400, 24000), "chr1": (gene_end["chr1"] - 700, gene_end["chr1"] - 400)}
    for name, (a, b) in n_runs.items():
        seqs[name][a:b] = ord("N")

    genes, txs = [], []
    for name in ("chr2", "chr10", "chr1", "MT", "chrX"):
        usable = gene_end[name] - 3600 - 1000
        g, t = synth.synth_annotation(rng, name, gene_end[name], 3600, max(2, usable // 3500))
        for x in t:
            x["id"] = name + "." + x["id"]
            x["gene_idx"] += len(genes)
        genes += [dict(id=name + "." + x["id"], name=name + "." + x["name"]) for x in g]
        txs += t
    hand = {}

    def gene(key, chrom, strand, exons):
        hand[key] = dict(gene=len(genes), tx=len(txs))
        genes.append(dict(id="HAND_" + key, name=key))
        txs.append(dict(id="HANDT_" + key, gene_idx=len(genes) - 1, chrom=chrom, strand=strand, exons=exons))

    def last(n):
        return [(n - 500, n - 300), (n - 150, n)]

    gene("first_fwd", "chr2", True, [(0, 150), (400, 600)])
    gene("last_rev", "chr2", False, last(36000))
    gene("last_fwd", "chr10", True, last(32000))
    gene("first_rev", "chr1", False, [(0, 150), (400, 600)])
    gene("in_paralog", "chr2", True, [(1500, 1700), (P1_AT + 300, P1_AT + 500), (P1_AT + P1_LEN + 50, P1_AT + P1_LEN + 150)])
    gene("whole_contig", SCAF_GENE_300, True, [(0, 300)])
    gene("short_tx", SCAF_SHORT_TX, True, [(10, 60)])
    t = refdata.build_tables([(name, seqs[name]) for name, _, _ in order], genes, txs)
    index_of = {name: i for i, (name, _, _) in enumerate(order)}
    info = dict(order=order, index_of=index_of, p1=p1, fam=fam, plants=plants, gene_end=gene_end, n_runs=n_runs, hand=hand,
                edge_genes=[hand[k]["gene"] for k in ("first_fwd", "last_rev", "last_fwd", "first_rev")],
                tx_contig=np.array([index_of[x["chrom"]] for x in txs], np.int64),
                kind=np.array([k for _, _, k in order]), lens=np.array([n for _, n, _ in order], np.int64))
    return t, info


def world():
    """(tables, what was planted)"""
    if "world" not in _memo:
        _memo["world"] = _make()
    return _memo["world"]


def forward(t, ci):
    r = t["refs"][2 * ci]
    return t["text"][int(r["start_idx"]): int(r["start_idx"]) + int(r["len"])]


def contig_of(t, ref_id):
    """file index (BAM refID) of the contig of every thm_ref index in `ref_id`"""
    return t["refs"]["name_id"][np.asarray(ref_id, np.int64)].astype(np.int64)


def holds_alignment(t, info, ci, min_score=capi.CI_OPTS["min_aln_score"]):
    """the contig has min_seed_len bases for a seed and min_score bases for an alignment, not all of them N"""
    f = forward(t, ci)
    return len(f) >= max(K, min_score) and int((f != ord("N")).sum()) >= max(K, min_score)


# ------------------------------------------------------------------ reads
def _n_count(a):
    return int((np.asarray(a) == ord("N")).sum())


class _Reads:
    def __init__(self):
        self.seqs, self.kinds = [], []

    def add(self, kind, a, flip=False):
        a = np.ascontiguousarray(a, np.uint8)
        if _n_count(a) > 1:
            return False
        self.seqs.append(refdata.revcomp(a) if flip else a)
        self.kinds.append(kind)
        return True

    def both(self, kind, a):
        return self.add(kind, a) and self.add(kind, a, True)


def _transcript_reads(out, t, info, per_contig, stream0):
    """simulate_reads (no intronic fraction) over the transcripts of one annotated contig at a time"""
    for ci in np.unique(info["tx_contig"]):
        mask = info["tx_contig"] == ci
        if not (t["txs"]["seq_len"][mask] >= L0 + 2).any():
            continue
        bases, off, _ = synth.simulate_reads(dict(t, txs=t["txs"][mask]), per_contig, L0, sub_rate=0.01, indel_rate=0.001, stream=stream0 + int(ci))
        for i in range(per_contig):
            out.add("tx", bases[off[i]: off[i + 1]])


def _edge_gene_reads(out, t, info, step):
    """windows along the hand-made transcripts; the transcript shorter than a read as it is"""
    for key, h in info["hand"].items():
        tx = t["txs"][h["tx"]]
        seq = t["tx_seq"][int(tx["seq_off"]): int(tx["seq_off"]) + int(tx["seq_len"])]
        if len(seq) < L0:
            out.both("hand_" + key, seq)
            continue
        for k, s in enumerate(list(range(0, len(seq) - L0, step)) + [len(seq) - L0]):
            out.add("hand_" + key, seq[s: s + L0], flip=bool(k & 1))


def _genomic_reads(out, t, info, rng, density=200, cap=120):
    """per contig, from within its forward sequence: both orientations, light substitutions and indels"""
    for ci, n in enumerate(info["lens"]):
        f = forward(t, ci)
        if n < L0:
            continue
        for k in range(min(max(4, int(n) // density), cap)):
            for _ in range(4):   # (a window in an N run is drawn again)
                s = int(rng.integers(0, n - L0 + 1))
                if _n_count(f[s: s + L0]) <= 1:
                    out.add("genomic", mutate(rng, f[s: s + L0], sub=0.01, indel=0.002), flip=bool(k & 1))
                    break


def _paralog_tiling(out, t, info, rng, L, stride, kind=None):
    """windows of the paralogous segment as chr2 has it: exact and with one substitution, both orientations"""
    f = forward(t, info["index_of"]["chr2"])
    for k, s in enumerate(range(P1_AT, P1_AT + P1_LEN - L + 1, stride)):
        w = f[s: s + L]
        if k & 2:
            w = sf.substitute(w, int(rng.integers(K + 1, L - K - 1)), rng)
        out.add(kind or "p1_%d" % L, w, flip=bool(k & 1))


def _family_columns(t, info, fam):
    """the copies of a family, one row each, in the consensus's orientation"""
    if ("columns", fam) not in _memo:
        rows = [forward(t, info["index_of"][name])[at: at + FAM_LEN] for name, at, _ in info["plants"][fam]]
        _memo[("columns", fam)] = np.stack([r if fwd else refdata.revcomp(r) for r, (_, _, fwd) in zip(rows, info["plants"][fam])])
    return _memo[("columns", fam)]


def _family_reads(out, t, info, rng, fam, n):
    """91-base reads from the copies of a family, some with one substitution in the middle (two SMEMs).  Of the diverged
    family F3 every second read is cut from the consensus: a read from a copy holds that copy's own differences, and the
    SMEM through one of them occurs once; the two halves of a consensus window occur in every copy that has no difference
    there -- about half of the copies each, which is what gives a read TEAM_HITS seed hits and more."""
    pl = info["plants"][fam]
    for k in range(n):
        name, at, _ = pl[int(rng.integers(0, len(pl)))]
        s = at + int(rng.integers(0, FAM_LEN - L0 + 1))
        w = forward(t, info["index_of"][name])[s: s + L0]
        if fam == "F3" and (k & 2) == 0:
            # the substituted base is one that no copy has there: else the read would match that copy through the substitution
            c0 = s - at
            w = info["fam"][fam][c0: c0 + L0].copy()
            columns = _family_columns(t, info, fam)
            p, b = next((p, b) for p in (45, 44, 46, 43, 47, 42, 48) for b in _ACGT if not (columns[:, c0 + p] == b).any())
            w[p] = b
        elif fam == "F3" or (k & 2):
            w = sf.substitute(w, 45 + (k % 3), rng)
        out.add(fam, w, flip=bool(k & 1))


def _contig_end_reads(out, t, info, rng, contigs=None):
    """for every contig, both orientations: its last 60 bases and 31 random ones, 31 random ones and its first 60 bases, the
    whole contig between two random flanks (up to 200 bases), the contig itself (90, 91, 92 bases), and the end of the contig
    joined to the start of the next one in the file"""
    n_contigs = len(info["lens"])
    for ci in (range(n_contigs) if contigs is None else contigs):
        f = forward(t, ci)
        n = len(f)
        out.both("end_tail", np.concatenate([f[-60:], _rand(rng, L0 - min(n, 60))]))
        out.both("end_head", np.concatenate([_rand(rng, L0 - min(n, 60)), f[:60]]))
        if n <= 200:
            out.both("end_whole", np.concatenate([_rand(rng, 20), f, _rand(rng, 20)]))
        if n in (90, 91, 92):
            out.both("end_equal", f)
        if ci + 1 < n_contigs:
            out.both("end_join", np.concatenate([f[-45:], forward(t, ci + 1)[:46]]))


FINISHER_CONTIGS = ("chr10", "chr1", "MT", "chrX", "KI270_b", "chrUn_10", "scaf6", "scaf1", "scaf2", "scaf11")


def _exons_forward(t, ci):
    r = t["refs"][2 * ci]
    e = t["exons"]
    on = (e["start"] >= r["start_idx"]) & (e["end"] <= r["end_idx"])
    s = np.unique(np.stack([e["start"][on] - r["start_idx"], e["end"][on] - r["start_idx"]], axis=1).astype(np.int64), axis=0)
    return [(int(a), int(b)) for a, b in s if b - a >= L0]


def _finisher_reads(out, t, info, rng):
    """the finisher's two shapes (smem_finish.h: class E, whole-read exact; class S, one substitution between two SMEMs) on
    contigs other than the first: inside exons and flush with their ends, between the genes, and the first and last
    window of the contig"""
    ps = [20, 21, 45, L0 - 22, L0 - 21]
    for name in FINISHER_CONTIGS:
        ci = info["index_of"][name]
        f = forward(t, ci)
        n = len(f)
        starts = [0, 1, n - L0, n - L0 - 1]
        ex = _exons_forward(t, ci)
        for i in rng.permutation(len(ex))[:6]:
            a, b = ex[i]
            starts += [a, b - L0, a - 1, b - L0 + 1, a + int(rng.integers(0, b - a - L0 + 1))]
        if n > 2 * L0:
            starts += [int(v) for v in rng.integers(0, n - L0, 8)]
        for k, s in enumerate(sorted(set(s for s in starts if 0 <= s <= n - L0))):
            w = f[s: s + L0]
            if _n_count(w):
                continue
            out.add("fin_E", w, flip=bool(k & 1))
            out.add("fin_S", sf.substitute(w, ps[k % len(ps)], rng), flip=bool(k & 2))


def _ragged_reads(out, t, info, rng, n):
    for k in range(n):
        name, ln = LARGE[k % len(LARGE)]
        length = int(rng.integers(0, 301))
        s = int(rng.integers(0, ln - 300))
        out.add("ragged", mutate(rng, forward(t, info["index_of"][name])[s: s + length], sub=0.01, indel=0.002), flip=bool(k & 1))


def _finish(out, rng, n_every=0):
    """list of reads as bytes, in a fixed shuffled order; with n_every: an N into every n_every-th read that has none"""
    seqs = [np.array(s, np.uint8) for s in out.seqs]
    if n_every:
        for i in range(0, len(seqs), n_every):
            if len(seqs[i]) and _n_count(seqs[i]) == 0 and not out.kinds[i].startswith(("fin_", "n_run")):
                seqs[i][int(rng.integers(0, len(seqs[i])))] = ord("N")
    order = rng.permutation(len(seqs))
    return dict(seqs=[bytes(seqs[i]) for i in order], kinds=[out.kinds[i] for i in order])


def pack(rs):
    return refdata.pack_reads(rs["seqs"])


def _set(name):
    if name in _memo:
        return _memo[name]
    t, info = world()
    rng = np.random.Generator(np.random.PCG64([SEED, 2, sum(name.encode())]))
    out = _Reads()
    n_every = 0
    if name == "general":
        _transcript_reads(out, t, info, 250, 100)
        _edge_gene_reads(out, t, info, 9)
        _genomic_reads(out, t, info, rng)
        _paralog_tiling(out, t, info, rng, 91, 7)
        _paralog_tiling(out, t, info, rng, 150, 13)
        _paralog_tiling(out, t, info, rng, 300, 100)
        for fam, n in (("F2", 32), ("F3", 24), ("F4", 16)):
            _family_reads(out, t, info, rng, fam, n)
        _contig_end_reads(out, t, info, rng)
        _finisher_reads(out, t, info, rng)
        _ragged_reads(out, t, info, rng, 200)
        for _ in range(80):
            out.add("random", _rand(rng, L0))
        f = forward(t, info["index_of"]["chr2"])
        for s in (9000, 12000):     # two reads with a run of N: shorter than any seed on either side of it
            w = f[s: s + L0].copy()
            w[40:48] = ord("N")
            out.seqs.append(w)
            out.kinds.append("n_run")
        n_every = 20
    elif name == "list":      # more than KEYCAP accepted candidates per read, among ordinary reads
        _family_reads(out, t, info, rng, "F2", 60)
        _genomic_reads(out, t, info, rng, density=2000, cap=12)
    elif name == "team":      # at least TEAM_HITS seed hits per read; the heavy list (8 to 31 hits) beside them
        _family_reads(out, t, info, rng, "F3", 40)
        _family_reads(out, t, info, rng, "F4", 16)
        _genomic_reads(out, t, info, rng, density=2000, cap=12)
    elif name == "wide":      # 300 bases under WIDE_OPTS: the any-width kernel
        _paralog_tiling(out, t, info, rng, 300, 8, kind="p1_300")
        _ragged_reads(out, t, info, rng, 40)
    elif name == "per_hit":
        _contig_end_reads(out, t, info, rng, contigs=range(0, len(info["lens"]), 2))
        _paralog_tiling(out, t, info, rng, 91, 60)
        _family_reads(out, t, info, rng, "F4", 8)
        _edge_gene_reads(out, t, info, 40)
    elif name == "tiny":      # the contigs of fewer than 30 bases, each between two random flanks (TINY_OPTS)
        for ci in np.nonzero(info["lens"] < 30)[0]:
            f = forward(t, int(ci))
            out.both("tiny", np.concatenate([_rand(rng, 20), f, _rand(rng, 20)]))
            out.both("tiny", np.concatenate([f, _rand(rng, 25)]))
    else:
        raise KeyError(name)
    _memo[name] = _finish(out, rng, n_every)
    return _memo[name]


def read_set(name="general"):
    """dict(seqs: list of bytes, kinds: what each read was made as) -- 'general' (about 5000 reads, every kind), 'list',
    'team', 'wide', 'per_hit' and 'tiny' (a few hundred each, for one path)"""
    return _set(name)


# ------------------------------------------------------------------ idx_to_ref from the host tables
def ref_tables(ix):
    """(ref_bin, ref_recs as a structured array) of an index, as the kernels get them"""
    c = "<u8" if ix.coord_bytes == 8 else "<u4"
    rec_dt = np.dtype([("start", c), ("end", c), ("len", c), ("name_rank", "<u4"), ("strand", "<u4")])
    return ix.debug_host_table("ref_bin").view("<u4"), ix.debug_host_table("ref_recs").view(rec_dt)


def bin_and_walk(ref_bin, ref_recs, idx):
    """idx_to_ref as extend_device.h, kernels_hit.hip, kernels_tpr.hip and smem_finish.h state it -> (contig copy, steps walked)"""
    lo = int(ref_bin[idx >> GRID_SHIFT])
    steps = 0
    while int(ref_recs["end"][lo]) <= idx and lo + 1 < len(ref_recs):
        lo += 1
        steps += 1
    return lo, steps
