"""Shared helpers for the -m gpu parity tests (HIP path vs the CPU oracle)."""
import numpy as np

from oracle import pyoracle as orc
from thermite_amd import capi, refdata, synth

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def mutate(rng, a, sub=0.05, indel=0.02):
    out = []
    for ch in a:
        r = rng.random()
        if r < indel / 2:
            continue
        if r < indel:
            out.append(int(_ACGT[rng.integers(0, 4)]))
        if rng.random() < sub:
            out.append(int(_ACGT[rng.integers(0, 4)]))
        else:
            out.append(int(ch))
    return np.array(out, np.uint8)


def swg_fuzz_problems(rng, n, max_len, bw_lo, bw_hi, related=0.8):
    xs, ys, bws, xds = [], [], [], []
    for _ in range(n):
        xl = int(rng.integers(0, max_len + 1))
        x = _ACGT[rng.integers(0, 4, xl)]
        bw = int(rng.integers(bw_lo, bw_hi + 1))
        if rng.random() < related:
            y = mutate(rng, x, sub=rng.random() * 0.15, indel=rng.random() * 0.06)
            tail = _ACGT[rng.integers(0, 4, int(rng.integers(0, 40)))]
            y = np.concatenate([y, tail])
            if rng.random() < 0.2:
                y = y[: int(rng.integers(0, len(y) + 1))]
        else:
            y = _ACGT[rng.integers(0, 4, int(rng.integers(0, max_len + 40)))]
        xs.append(x)
        ys.append(y.astype(np.uint8))
        bws.append(bw)
        xds.append(bw + int(rng.integers(0, 4)) * int(rng.integers(0, 8)))
    xb, xo = refdata.pack_reads(xs)
    yb, yo = refdata.pack_reads(ys)
    return xb, xo, yb, yo, np.array(bws, "<u4"), np.array(xds, "<i4")


def assert_swg_equal(gpu_alns, gpu_ops, ref):
    assert len(gpu_alns) == len(ref.swg)
    for f in ("score", "xend", "yend", "ops_len", "ops_off"):
        bad = np.nonzero(gpu_alns[f] != ref.swg[f])[0]
        assert len(bad) == 0, "field %s differs at problems %s" % (f, bad[:10])
    assert np.array_equal(gpu_ops, ref.ops)


def assert_batch_equal(gpu, ref, max_report=5):
    """gpu: capi.BatchResult, ref: oracle Result('aln') -- canonical layouts must be byte-identical."""
    assert gpu.n_reads == ref.n
    if not np.array_equal(gpu.offsets, ref.offsets):
        d = np.nonzero(np.diff(gpu.offsets.astype(np.int64)) != np.diff(ref.offsets.astype(np.int64)))[0]
        raise AssertionError("alignment counts differ for reads %s" % d[:max_report])
    for f in capi.ALN_DT.names:
        if f == "pad_":
            continue
        bad = np.nonzero(gpu.alns[f] != ref.alns[f])[0]
        if len(bad):
            i = int(bad[0])
            read = int(np.searchsorted(ref.offsets, i, side="right") - 1)
            raise AssertionError("field %s differs at alignment %d (read %d): gpu=%s ref=%s" %
                                 (f, i, read, gpu.alns[i], ref.alns[i]))
    assert np.array_equal(gpu.ops, ref.ops), "op streams differ"


class World:
    """An index of the product (32- or 64-bit coordinates) and the oracle's index over the same tables and suffix array."""

    def __init__(self, tables, wide=False):
        self.t = tables
        self.ix = capi.Index(tables, wide=wide)
        assert self.ix.coord_bytes == (8 if wide else 4)
        self.oix = orc.Index(tables, sa=self.ix.suffix_array())
        self._a = None

    @property
    def a(self):
        """a long-lived aligner with the CI options (the per-hit entry points take their band per hit)"""
        if self._a is None:
            self._a = capi.Aligner(self.ix, capi.CI_OPTS)
        return self._a

    def aligner(self, opts):
        return capi.Aligner(self.ix, opts)


def check_smems(w, bases, off, k):
    a = w.aligner(dict(capi.DEFAULT_OPTS, min_seed_len=k))
    g_off, g_mems = a.smems_batch(bases, off, k)
    r = w.oix.all_smems(bases, off, k)
    assert np.array_equal(g_off, r.offsets)
    for f in ("ref_idx", "query_idx", "len"):
        bad = np.nonzero(g_mems[f] != r.mems[f])[0]
        assert len(bad) == 0, "%s differs at mem %d" % (f, bad[0])
    a.close()


def assert_counters_match(c, rc, what=""):
    """device counters against the oracle's after one batch"""
    assert np.array_equal(c[:10], rc[:10]) and c[12] == rc[12] and c[13] == rc[13], (what, c[:14], rc[:14])
    assert c[10] <= rc[10] and c[11] <= rc[11], (what, c[:14], rc[:14])  # DP work: exact early exit computes fewer cells


def check_align(w, bases, off, opts, n_threads=8, pool_caps=None, ref=None):
    """Both device paths against the oracle: the problem-parallel path (kernels_tpr.hip: thread-per-read control
    kernel + wave-per-request DP kernel; what it leaves goes to the wave-per-read kernels) and the wave-per-read
    kernels alone.  pool_caps: arguments of debug_set_pool_caps, pools so small that the batch must overflow, grow
    and replay (asserted); ref: the oracle's result, where the caller has it already."""
    r = ref if ref is not None else w.oix.align_batch(bases, off, opts, n_threads=n_threads)
    assert r.counters[15] == 0, "oracle saw reads where the reference would panic"
    g = None
    for no_tpr in (False, True):
        a = w.aligner(opts)
        a.debug_set_flags(tpr=not no_tpr)
        replays = a.debug_set_pool_caps(**pool_caps) if pool_caps else None
        a.reset_counters()
        g = a.align_batch(bases, off)
        if pool_caps:
            assert a.debug_set_pool_caps() > replays, "the small pools did not overflow: %r" % (pool_caps,)
        assert g.n_failed == 0 and g.status is None
        assert_batch_equal(g, r)
        assert_counters_match(a.counters(), r.counters, no_tpr)
        a.close()
    return g


ALN_EXONIC, ALN_INTRONIC, ALN_INTERGENIC = 0, 1, 2  # AlnType, include/thermite.h


# ------------------------------------------------------------------ restatement of align_seed_hit
def _idx_to_ref(refs, idx):  # Index::idx_to_ref, src/index.rs:287-290: refs.partition_point(|x| x.end_idx <= idx)
    return int(np.searchsorted(refs["end_idx"], idx, side="right"))


def _tx_exons(t, tx_idx):
    tx = t["txs"][tx_idx]
    ex = t["exons"][int(tx["exon_begin"]): int(tx["exon_begin"]) + int(tx["n_exons"])]
    return [(int(e["start"]), int(e["end"]), int(tx_idx)) for e in ex]


def _tx_seq(t, tx_idx):
    tx = t["txs"][tx_idx]
    return t["tx_seq"][int(tx["seq_off"]): int(tx["seq_off"]) + int(tx["seq_len"])]


def _concat_to_chr(refs, ystart, yend, ops):  # src/aligner.rs:429-449
    r = refs[_idx_to_ref(refs, ystart)]
    s0, ln = int(r["start_idx"]), int(r["len"])
    if r["strand"]:
        return ystart - s0, yend - s0, ln, ops
    return ln - (yend - s0), ln - (ystart - s0), ln, list(reversed(ops))


def expected_hit(w, swg, read, hit, bw, xd):
    """align_seed_hit, src/aligner.rs:198-314: one ALN_DT record (primary 0) and its op bytes (gx, then tx), or raises
    RuntimeError where the reference panics in a lift."""
    t, oix = w.t, w.oix
    refs, text = t["refs"], t["text"]
    L = len(read)
    hr, q, ln = hit
    k = _idx_to_ref(refs, hr)
    ref = refs[k]
    seq_start = max(max(hr - (L + bw), 0), int(ref["start_idx"]))
    seq_end = min(hr + ln + L + bw, int(ref["end_idx"]) - 1)
    g = swg.extend_left_right(text[seq_start:seq_end], (hr - seq_start, q, ln), read, bw, xd)
    g["ystart"] += seq_start
    g["yend"] += seq_start
    best = None
    for tx_idx in oix.exon_tree_find(hr, hr + ln):
        exons = _tx_exons(t, tx_idx)
        seq = _tx_seq(t, tx_idx)
        seed = orc.lift_mem_to_tx((hr, q, ln), exons)
        seed = orc.extend_seed_match(seq, seed, read)
        a = swg.extend_left_right(seq, seed, read, bw, xd)
        if best is None or a["score"] > best[1]["score"]:
            best = (tx_idx, a)
        if a["score"] >= L:
            break
    rec = np.zeros(1, capi.ALN_DT)[0]
    rec["ref_id"], rec["strand"], rec["primary"], rec["xlen"] = k, ref["strand"], 0, L
    if best is not None and best[1]["score"] >= g["score"]:
        tx_idx, a = best
        lifted = orc.lift_tx_to_gx(a["ops"], a["ystart"], a["yend"], _tx_exons(t, tx_idx))
        ys, ye, ylen, ops = _concat_to_chr(refs, lifted["ystart"], lifted["yend"], lifted["ops"])
        gx_bytes, tx_bytes = orc.encode_ops(ops), orc.encode_ops(a["ops"])
        rec["aln_type"], rec["tx_or_gene_idx"] = ALN_EXONIC, tx_idx
        rec["score"], rec["xstart"], rec["xend"] = a["score"], a["xstart"], a["xend"]
        rec["tx_ystart"], rec["tx_yend"], rec["tx_ylen"] = a["ystart"], a["yend"], a["ylen"]
        rec["tx_score"], rec["tx_xstart"], rec["tx_xend"], rec["tx_ops_len"] = a["score"], a["xstart"], a["xend"], len(tx_bytes)
    else:
        genes = oix.gene_tree_find(g["ystart"], g["yend"])
        ys, ye, ylen, ops = _concat_to_chr(refs, g["ystart"], g["yend"], g["ops"])
        gx_bytes, tx_bytes = orc.encode_ops(ops), b""
        rec["aln_type"] = ALN_INTRONIC if genes else ALN_INTERGENIC
        rec["tx_or_gene_idx"] = genes[0] if genes else 0xFFFFFFFF
        rec["score"], rec["xstart"], rec["xend"] = g["score"], g["xstart"], g["xend"]
    rec["ystart"], rec["yend"], rec["ylen"], rec["ops_len"] = ys, ye, ylen, len(gx_bytes)
    return rec, gx_bytes + tx_bytes


def expected_batch(w, bases, off, hit_off, hits, bw, xd, max_bw):
    """records, op bytes (canonical layout) and statuses the restatement gives for every hit"""
    swg = orc.Swg(max_bw)
    recs = np.zeros(len(hits), capi.ALN_DT)
    ops = bytearray()
    status = np.zeros(len(hits), "<i4")
    for r in range(len(off) - 1):
        read = bytes(bases[off[r]: off[r + 1]]).upper()
        for h in range(int(hit_off[r]), int(hit_off[r + 1])):
            m = hits[h]
            try:
                rec, b = expected_hit(w, swg, read, (int(m["ref_idx"]), int(m["query_idx"]), int(m["len"])), int(bw[h]), int(xd[h]))
            except RuntimeError:
                status[h] = capi.ERR_OUT_OF_CONTRACT
                continue
            rec["ops_off"] = len(ops)
            if rec["aln_type"] == ALN_EXONIC:
                rec["tx_ops_off"] = len(ops) + rec["ops_len"]
            ops += b
            recs[h] = rec
    return recs, np.frombuffer(bytes(ops), np.uint8), status


def assert_hits_equal(got, exp, what=""):
    g_alns, g_ops, g_st = got
    e_alns, e_ops, e_st = exp
    assert np.array_equal(g_st, e_st), (what, np.nonzero(g_st != e_st)[0][:10], g_st[g_st != e_st][:10], e_st[g_st != e_st][:10])
    for f in capi.ALN_DT.names:
        bad = np.nonzero(g_alns[f] != e_alns[f])[0]
        if len(bad):
            i = int(bad[0])
            raise AssertionError("%s field %s differs at hit %d: gpu=%s expected=%s" % (what, f, i, g_alns[i], e_alns[i]))
    assert np.array_equal(g_ops, e_ops), what + ": op streams differ"


def initial_band(opts, L):  # align_read's initial band and X-drop, src/aligner.rs:130-138
    ms = max(int(np.float32(opts["min_aln_score_percent"]) * np.float32(L)), opts["min_aln_score"])
    return max(L - ms, 0) if ms >= 0 else L


# ------------------------------------------------------------------ micro-exon reference
# Transcripts with hundreds of exons of 1-3 bases: an alignment along one of them crosses more introns than the
# register-resident extend kernels keep markers for (FAST_MAX_YCLIPS = 64, extend_plan.h), so its read is handed to the
# any-width kernel (the retry list).  Nothing else in the suite has a transcript of more than 11 exons.
MICRO_SLOT = 10000      # contig bases reserved per micro-exon transcript
MICRO_TERMINAL = 60     # first and last exon: long enough for a genomic seed
MICRO_PLANT_TAIL = 12   # genomic bases behind the planted first exon (see micro_exon_reference)
MICRO_OPTS = dict(min_seed_len=12, min_aln_score_percent=0.66, min_aln_score=30, multimap_score_range=1, intron_mode=True)
MARKER_LIMIT = 64       # FAST_MAX_YCLIPS


def micro_exon_reference(n_micro=6, n_genes=10, gene_region=60000, n_plant=0, with_micro=True, seed=0x6D6963726F):
    """One random ACGT contig laid out as [micro-exon transcripts | ordinary multi-exon genes | planted copies].

    Micro-exon transcript k (strand '+' for even k) has a first exon of 60 bases, 70..200 exons of 1, 2 or 3 bases
    separated by introns of 30..50 bases, and a last exon of 60 bases.  Transcripts 0 and 1 have micro-exons of one base
    only, so that a 91-base read can cross more than 64 introns.  `n_plant` copies of transcript 0's first exon and the
    MICRO_PLANT_TAIL genomic bases behind it go into the last region: a read that starts in that exon has an SMEM with
    n_plant + 1 occurrences (the tail keeps the chance extension of the match into the first intron common to all copies;
    the bare 60-mer would be contained in a longer, unique match at the transcript itself and not be an SMEM).
    with_micro=False: the same contig and the same ordinary genes, without the micro-exon transcripts.
    The ordinary genes and their transcripts come first in the tables, so their indices agree between the two.
    Returns the tables; tables["_micro"] lists the micro-exon transcripts as dict(tx_idx, strand, exons)."""
    rng = np.random.Generator(np.random.PCG64([seed, n_micro, n_genes, n_plant]))
    micro_len = n_micro * MICRO_SLOT
    plant_unit = MICRO_TERMINAL + MICRO_PLANT_TAIL
    length = micro_len + gene_region + n_plant * (plant_unit + 40) + 200
    seq = _ACGT[rng.integers(0, 4, length)]
    name = "microsyn"
    micro = []
    for k in range(n_micro):
        n_ex = [200, 130, 70, 200, 101, 160][k] if k < 6 else int(rng.integers(70, 201))
        sizes = np.ones(n_ex, np.int64) if k < 2 else rng.integers(1, 4, n_ex)
        introns = rng.integers(30, 51, n_ex + 1)
        p = k * MICRO_SLOT + 200 + int(rng.integers(0, 200))
        exons = [(p, p + MICRO_TERMINAL)]
        p += MICRO_TERMINAL
        for j in range(n_ex):
            p += int(introns[j])
            exons.append((p, p + int(sizes[j])))
            p += int(sizes[j])
        p += int(introns[n_ex])
        exons.append((p, p + MICRO_TERMINAL))
        assert p + MICRO_TERMINAL < (k + 1) * MICRO_SLOT
        micro.append(dict(strand=(k % 2 == 0), exons=exons))
    if n_plant:
        a = micro[0]["exons"][0][0]
        unit = seq[a: a + plant_unit].copy()
        p = micro_len + gene_region + 100
        for _ in range(n_plant):
            seq[p: p + plant_unit] = unit
            p += plant_unit + int(rng.integers(20, 41))
        assert p < length
    genes, txs = synth.synth_annotation(rng, name, micro_len + gene_region, micro_len, n_genes)
    if with_micro:
        for k, m in enumerate(micro):
            m["tx_idx"] = len(txs)
            genes.append(dict(id="MICG%03d" % k, name="micro%d" % k))
            txs.append(dict(id="MICT%03d" % k, gene_idx=len(genes) - 1, chrom=name, strand=m["strand"], exons=m["exons"]))
    t = refdata.build_tables([(name, seq)], genes, txs)
    t["_micro"] = micro if with_micro else []
    t["_gene_region"] = (micro_len, micro_len + gene_region)
    return t


def count_yclips(res, i):
    """intron markers in the genomic op stream of alignment i of an oracle (or device) result"""
    a = res.alns[i]
    ops = orc.decode_ops(res.ops[int(a["ops_off"]): int(a["ops_off"]) + int(a["ops_len"])])
    return sum(1 for o in ops if isinstance(o, tuple) and o[0] == "Yclip")


def exonic_yclip_counts(res):
    """Yclip ops of every final exonic alignment of a read-level result"""
    return np.array([count_yclips(res, i) for i in np.nonzero(res.alns["aln_type"] == ALN_EXONIC)[0]], np.int64)


def _micro_windows(t, m, L, min_anchor=14):
    """(start in transcript coordinates, introns crossed) of every L-base window of micro-exon transcript m that has at
    least min_anchor bases in a terminal exon -- the genomic seed; a window inside the micro-exon stretch has none"""
    tx = t["txs"][m["tx_idx"]]
    n = int(tx["n_exons"])
    ex = t["exons"][int(tx["exon_begin"]): int(tx["exon_begin"]) + n]
    lens = (ex["end"] - ex["start"]).astype(np.int64)
    first = np.cumsum(lens) - lens       # transcript coordinate of each exon's first base
    tl = int(lens.sum())
    out = []
    for s in range(0, tl - L + 1):
        e = s + L
        if not (s + min_anchor <= int(lens[0]) or e - min_anchor >= int(first[-1])):
            continue
        k = int(np.searchsorted(first, e - 1, side="right") - np.searchsorted(first, s, side="right"))
        out.append((s, k))
    return out


def _edit(read, p, kind, rng):
    """one edit at read position p: a substitution, an inserted base in front of p, or p deleted"""
    r = list(read)
    if kind == "sub":
        r[p] = int(_ACGT[(int(np.nonzero(_ACGT == r[p])[0][0]) + 1 + int(rng.integers(0, 3))) % 4])
    elif kind == "ins":
        r.insert(p, int(_ACGT[rng.integers(0, 4)]))
    else:
        del r[p]
    return np.array(r, np.uint8)


def micro_exon_reads(t, lengths=(91, 150, 200, 250), mutated=False, stride=7, seed=1):
    """Reads cut from the micro-exon transcripts of `t`, both orientations: every window that crosses 62..67 introns
    (both sides of the marker limit, placed and not left to chance) and every `stride`-th of the others.
    mutated=True: each window additionally with one substitution, one inserted and one deleted base -- at the first
    micro-exon boundary the read crosses, in the middle of the micro-exon stretch (where every base is at or next to an
    exon boundary) and, for every third window, spread by `mutate` -- so the ops come from the DP and not from the
    exact-match shortcut.  The bases of the terminal exon (the seed) stay as they are, except under `mutate`.
    Returns (bases, offsets, planned crossings per read [of the unedited window])."""
    rng = np.random.default_rng(seed)
    reads, planned = [], []
    n = 0
    for m in t["_micro"]:
        tx = t["txs"][m["tx_idx"]]
        seq = t["tx_seq"][int(tx["seq_off"]): int(tx["seq_off"]) + int(tx["seq_len"])]
        tl = len(seq)
        for L in lengths:
            for s, k in _micro_windows(t, m, L):
                near = MARKER_LIMIT - 2 <= k <= MARKER_LIMIT + 3
                if not near and (s % stride):
                    continue
                w = seq[s: s + L]
                # the read's part outside the terminal exon it is anchored in
                if s < MICRO_TERMINAL:
                    lo, hi = MICRO_TERMINAL - s, L
                else:
                    lo, hi = 0, (tl - MICRO_TERMINAL) - s
                variants = [w]
                if mutated:
                    variants = []
                    edge = lo if s < MICRO_TERMINAL else hi - 1
                    mid = (lo + hi) // 2
                    kinds = ("sub", "ins", "del")
                    variants.append(_edit(w, edge, kinds[n % 3], rng))
                    variants.append(_edit(w, mid, kinds[(n + 1) % 3], rng))
                    if near:
                        variants.append(_edit(w, min(max(mid + int(rng.integers(-9, 10)), lo), hi - 1), kinds[(n + 2) % 3], rng))
                    if n % 3 == 0:
                        variants.append(mutate(rng, w, sub=0.03, indel=0.01))
                for v in variants:
                    reads.append(refdata.revcomp(v) if (n % 4 == 3) else v)  # (the opposite strand has no transcript: genomic hits only)
                    planned.append(k)
                    n += 1
    bases, off = refdata.pack_reads(reads)
    return bases, off, np.array(planned, np.int64)


def ordinary_reads(t, n, L=91, stream=0, sub_rate=0.01, indel_rate=0.001):
    """reads from the ordinary genes' transcripts and from the contig around them; none from a micro-exon transcript"""
    lo, hi = t["_gene_region"]
    n_tx = len(t["txs"]) - len(t["_micro"])
    sub = dict(t, txs=t["txs"][:n_tx])
    bases, off, _ = synth.simulate_reads(sub, n, L, sub_rate=sub_rate, indel_rate=indel_rate, stream=stream)
    reads = [bases[off[i]: off[i + 1]] for i in range(n)]
    rng = np.random.default_rng(stream + 17)
    fwd = t["text"][: int(t["refs"][0]["len"])]
    for i in range(0, n, 4):   # a quarter unspliced, from the genes' region of the contig
        s = int(rng.integers(lo, hi - L))
        g = mutate(rng, fwd[s: s + L], sub=sub_rate, indel=indel_rate)
        reads[i] = refdata.revcomp(g) if (i & 4) else g
    return refdata.pack_reads(reads)


# ------------------------------------------------------------------ more hits than the team kernel takes
TEAM_HITS, TEAM_MAX_HITS, COMPACT_HEAVY_N = 256, 60000, 8  # launch.h, kernels_compact.hip


def _other_base(*avoid):
    return int([b for b in _ACGT if int(b) not in [int(a) for a in avoid]][0])


def beyond_team_reference(n_full=TEAM_MAX_HITS, n_cut39=1, n_cut30=200, n_second=1000, n_genes=12, gene_region=200000, seed=0x626579):
    """A contig with an exact 40-mer U planted n_full times, once more cut to its first 39 bases and n_cut30 times cut to
    its first 30, a second 40-mer V planted n_second times, and two 120-mers planted 8 and 9 times.  Every copy stands
    between fixed bases (the base in front is the same for all copies, the base behind is the same within a kind), so a read
    that holds a prefix of U between *other* bases has that prefix as an SMEM with a known number of occurrences:
    U[:40] n_full, U[:39] n_full + n_cut39, U[:30] n_full + n_cut39 + n_cut30.  Ordinary genes fill the first region.
    Returns (tables, dict of the planted sequences and flank bases)."""
    rng = np.random.Generator(np.random.PCG64([seed, n_full, n_second]))
    U = _ACGT[rng.integers(0, 4, 40)]
    V = _ACGT[rng.integers(0, 4, 40)]
    fam = [_ACGT[rng.integers(0, 4, 120)] for _ in range(2)]
    front = int(_ACGT[0])
    behind40 = _other_base()                    # behind a whole copy
    behind39 = _other_base(U[39])               # behind a copy cut to 39 bases: not U[39]
    behind30 = _other_base(U[30])
    chunks = [_ACGT[rng.integers(0, 4, gene_region)]]
    kinds = [(U, behind40)] * n_full + [(U[:39], behind39)] * n_cut39 + [(U[:30], behind30)] * n_cut30 + [(V, behind40)] * n_second
    for i in rng.permutation(len(kinds)):
        body, b = kinds[i]
        chunks += [np.array([front], np.uint8), body, np.array([b], np.uint8), _ACGT[rng.integers(0, 4, int(rng.integers(18, 29)))]]
    for f, copies in zip(fam, (COMPACT_HEAVY_N, COMPACT_HEAVY_N + 1)):
        for _ in range(copies):
            chunks += [f, _ACGT[rng.integers(0, 4, 200)]]
    seq = np.concatenate(chunks).astype(np.uint8)
    genes, txs = synth.synth_annotation(rng, "beyond", gene_region, 500, n_genes)
    t = refdata.build_tables([("beyond", seq)], genes, txs)
    t["_gene_region"] = (500, gene_region - 1000)
    t["_micro"] = []
    info = dict(U=U, V=V, fam=fam, front=front, behind={40: behind40, 39: behind39, 30: behind30})
    return t, info


def beyond_team_reads(info, rng, n_each=2):
    """91-base reads whose only long SMEM is a prefix of U (40, 39 or 30 bases) or V, between bases no copy has next to
    it, and reads from the two small families.  Returns (list of reads, list of kinds: 'U40', 'U39', 'U30', 'V', 'F8', 'F9')."""
    U, V = info["U"], info["V"]
    reads, kinds = [], []

    def around(body, next_in_copies, kind):
        for j in range(n_each):
            left = int(rng.integers(10, 91 - len(body) - 10))
            l = _ACGT[rng.integers(0, 4, left)].copy()
            r = _ACGT[rng.integers(0, 4, 91 - len(body) - left)].copy()
            l[-1] = _other_base(info["front"])
            r[0] = _other_base(*next_in_copies)
            reads.append(np.concatenate([l, body, r]).astype(np.uint8))
            kinds.append(kind)

    around(U, [info["behind"][40]], "U40")
    around(U[:39], [U[39], info["behind"][39]], "U39")
    around(U[:30], [U[30], info["behind"][30]], "U30")
    around(V, [info["behind"][40]], "V")
    for f, kind in zip(info["fam"], ("F8", "F9")):
        for j in range(n_each):
            s = int(rng.integers(0, 120 - 91))
            reads.append(f[s: s + 91])
            kinds.append(kind)
    return reads, kinds
