"""Workloads of tests/test_gpu_knobs.py, shared with tests/knob_child.py: the parent (oracle, comparison) and the child
(one device run in a fresh process, under a run-time knob of INTEGRATION.md section 6) build identical inputs from fixed
seeds.

A workload is a dict: tables (the reference, None for the operator-level `swg`), runs (a list of dicts) and, for
`swg`, problem sets.  A read-level run has bases, off, opts, smem_k (min_seed_len of a thm_smems_batch call in front of
the alignment, or None), second (None, or another batch (bases, off) the same aligner aligns afterwards) and optionally
smem_reads (the oracle's SMEMs are computed and compared for that many reads at the front of the batch only)."""
import os

import numpy as np

from thermite_amd import capi, refdata, synth

from gpu_common import swg_fuzz_problems

_ACGT = np.frombuffer(b"ACGT", np.uint8)
_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
N_CU_DEFAULT = 256  # MI355X; the compact workload is sized from the knob report of the device it runs on
FAM_LEN = 120


def _run(bases, off, opts, smem_k=None, second=None):
    return dict(bases=bases, off=off, opts=opts, smem_k=smem_k, second=second)


def reversed_batch(bases, off):
    """the same reads in the opposite order: every per-read buffer of the aligner gets other contents"""
    off = off.astype(np.int64)
    return refdata.pack_reads([bases[off[i]: off[i + 1]] for i in range(len(off) - 2, -1, -1)]) if len(off) > 1 else (bases, off.astype("<u8"))


def planted_reference(copies, n_genes, gene_region, seed):
    """A random contig: ordinary multi-exon genes in the first `gene_region` bases, then for each entry of `copies` an
    exact FAM_LEN-mer planted that many times, 200 random bases apart (as beyond_team_reference plants its families): a
    read from inside family f has one SMEM with copies[f] occurrences and, under the CI options, copies[f] alignments.
    Returns tables; tables["_fam"] holds the planted sequences."""
    rng = np.random.Generator(np.random.PCG64([seed, len(copies), n_genes]))
    fam = [_ACGT[rng.integers(0, 4, FAM_LEN)] for _ in copies]
    chunks = [_ACGT[rng.integers(0, 4, gene_region)]]
    for f, c in zip(fam, copies):
        for _ in range(c):
            chunks += [f, _ACGT[rng.integers(0, 4, 200)]]
    seq = np.concatenate(chunks).astype(np.uint8)
    genes, txs = synth.synth_annotation(rng, "planted", gene_region, 500, n_genes)
    t = refdata.build_tables([("planted", seq)], genes, txs)
    t["_fam"] = fam
    t["_gene_region"] = (500, gene_region - 1000)
    return t


# ------------------------------------------------------------------ fill: THM_SEED_FILL
def _dirty_bytes(rng, b):
    b = b.copy()
    b[rng.random(len(b)) < 0.004] = ord("N")
    lower = rng.random(len(b)) < 0.2
    b[lower] = np.where((b[lower] >= 65) & (b[lower] <= 90), b[lower] + 32, b[lower])
    return b


def fill_workload():
    t = synth.synth_reference(length=300000, n_genes=30)
    runs = []
    too_short = None
    for k in (12, 20):
        rng = np.random.default_rng(100 + k)
        bases, off, _ = synth.simulate_reads(t, 2400, 120, sub_rate=0.02, indel_rate=0.004, intronic_frac=0.3, stream=500 + k)
        bases = _dirty_bytes(rng, bases)
        # every length from 0 up: below k, k and k + 1 (at most one position, nothing to probe), all residues of the
        # probe stride, and whole reads
        lens = np.where(np.arange(2400) % 3 == 0, 120, rng.integers(0, 121, 2400))
        lens[:64] = np.arange(64) % (k + 10)
        reads = [bases[int(off[i]): int(off[i]) + int(lens[i])] for i in range(2400)]
        lb, lo, _ = synth.simulate_reads(t, 60, 300, sub_rate=0.02, indel_rate=0.004, intronic_frac=0.3, stream=520 + k)
        lb = _dirty_bytes(rng, lb)
        for i in range(60):  # the long class, ragged
            reads.insert(int(rng.integers(0, len(reads) + 1)), lb[int(lo[i]): int(lo[i]) + (300 if i % 2 else int(rng.integers(256, 301)))])
        for i in range(0, 200, 5):  # N and lower case at the ends
            r = reads[i].copy()
            if len(r) > 2:
                r[0], r[-1] = ord("N"), ord("a") if r[-1] == ord("A") else ord("N")
            reads[i] = r
        short = [bases[j * 120: j * 120 + n] for j, n in enumerate((k - 1, k, k + 1, 3, 0, k + 2, k))]
        if k == 20:
            too_short = short
        reads += short  # the batch ends with reads of about k bases: the key kernel loads 8 bytes at each probe position
        b2, o2 = refdata.pack_reads(reads)
        runs.append(_run(b2, o2, dict(capi.CI_OPTS, min_seed_len=k), smem_k=k, second=reversed_batch(b2, o2)))
    ts = [r[: min(len(r), 21)] for r in too_short * 40]  # at most min_seed_len + 1 bases: the cell kernels run and list nothing
    b3, o3 = refdata.pack_reads(ts)
    runs.append(_run(b3, o3, capi.CI_OPTS, smem_k=20, second=(b3, o3)))
    empty = (np.zeros(0, np.uint8), np.zeros(1, "<u8"))
    runs.append(_run(empty[0], empty[1], capi.CI_OPTS, smem_k=20, second=empty))
    # More listed cells than the fixed grid of modes 1 and 2 has threads (FILL_FIXED_THREADS, launch_seed in
    # kernels_seed.hip): every kernel of the fill stage takes a second trip through its grid-stride loop.  A cell is
    # listed when the k-mer at its first position occurs nowhere in the text, so random reads list nearly all of theirs.
    rng = np.random.default_rng(112)
    nb, no, _ = synth.simulate_reads(t, FILL_BIG_NOISY, 120, sub_rate=0.10, indel_rate=0.01, intronic_frac=0.3, stream=540)
    nb = _dirty_bytes(rng, nb).reshape(FILL_BIG_NOISY, 120)
    big = _ACGT[rng.integers(0, 4, (FILL_BIG_RANDOM + FILL_BIG_NOISY, 120))]
    big[::(FILL_BIG_RANDOM + FILL_BIG_NOISY) // FILL_BIG_NOISY][:FILL_BIG_NOISY] = nb
    b4 = np.ascontiguousarray(big.reshape(-1))
    o4 = (np.arange(len(big) + 1, dtype=np.uint64) * np.uint64(120)).astype("<u8")
    runs.append(_run(b4, o4, dict(capi.DEFAULT_OPTS, min_seed_len=FILL_BIG_K), smem_k=FILL_BIG_K))
    runs[-1]["smem_reads"] = FILL_BIG_SMEM_READS
    return dict(tables=t, runs=runs)


FILL_FIXED_THREADS = 256 * 8 * 4 * 256  # the fixed grid: 8192 workgroups of 256 threads, one thread per slot of a cell
PROBE_STRIDE = 8                        # slots per cell, kernels_seed.hip
FILL_BIG_RANDOM, FILL_BIG_NOISY, FILL_BIG_K = 24000, 4000, 12
FILL_BIG_SMEM_READS = 1500  # reads of the big run whose SMEMs are compared (the oracle's seed pass runs on one thread)


def fill_listed_cells_at_least(tables, bases, off, k):
    """A lower bound of the cells seed_cells_kernel lists for the fill stage: cells c >= 1 with inner positions whose
    first position c * 8 holds an ACGT k-mer that occurs nowhere in the text (its matching statistic is below k, so
    ms_end is 0 there and the cell cannot be skipped).  k <= 13."""
    code = np.full(256, 4, np.int64)
    code[_ACGT] = np.arange(4)
    code[np.frombuffer(b"acgt", np.uint8)] = np.arange(4)  # reads are upper-cased on the device

    def kmers(a):  # (k-mer code, valid) per start position
        c = code[a]
        n = len(c) - k + 1
        v = np.zeros(n, np.int64)
        ok = np.ones(n, bool)
        for j in range(k):
            v = v * 4 + (c[j: j + n] & 3)
            ok &= c[j: j + n] < 4
        return v, ok

    tv, tok = kmers(tables["text"])
    present = np.zeros(4 ** k, bool)
    present[tv[tok]] = True
    rv, rok = kmers(bases)
    off = off.astype(np.int64)
    n = 0
    for r in range(len(off) - 1):
        npos = int(off[r + 1] - off[r]) - k + 1
        a = np.arange(PROBE_STRIDE, max(npos - 2, 0), PROBE_STRIDE)  # b - a > 1 with b = min(a + 8, npos - 1)
        if len(a):
            q = off[r] + a
            n += int((rok[q] & ~present[rv[q]]).sum())
    return n


# ------------------------------------------------------------------ compact: THM_COMPACT_K
COMPACT_COPIES = (2, 3, 8, 9)
COMPACT_KINDS = 7  # period of the interleaving; coprime to n_groups = n_cu * 128, so chains k and k + 1 of one group differ


def compact_n_reads(n_cu):
    return 3 * n_cu * 128 + 16 * 5 + 7


def compact_workload(n_cu=N_CU_DEFAULT):
    """kinds by batch position i % 7: 0, 3 ordinary reads (transcripts and contig), 1 random (no alignment), 2 / 4 / 5 / 6
    reads from the families of 2 / 8 / 9 / 3 copies; ragged lengths 60..120"""
    t = planted_reference(COMPACT_COPIES, n_genes=12, gene_region=120000, seed=0x636F6D70)
    n = compact_n_reads(n_cu)
    rng = np.random.default_rng(77)
    bases, off, _ = synth.simulate_reads(t, n, 120, sub_rate=0.01, indel_rate=0.001, intronic_frac=0.4, stream=601)
    arr = bases.reshape(n, 120).copy()
    kind = np.arange(n) % COMPACT_KINDS
    m = kind == 1
    arr[m] = _ACGT[rng.integers(0, 4, (int(m.sum()), 120))]
    lens = rng.integers(60, 121, n)
    for kd, f in ((2, 0), (6, 1), (4, 2), (5, 3)):
        fam = t["_fam"][f]
        idx = np.nonzero(kind == kd)[0]
        start = (rng.random(len(idx)) * (FAM_LEN - lens[idx] + 1)).astype(np.int64)
        win = np.concatenate([fam, fam])[start[:, None] + np.arange(120)[None, :]]  # (bases past the read's length are cut off)
        flip = rng.random(len(idx)) < 0.5
        for j in np.nonzero(flip)[0]:
            L = int(lens[idx[j]])
            win[j, :L] = refdata.revcomp(win[j, :L])
        arr[idx] = win
    keep = np.arange(120)[None, :] < lens[:, None]
    b2 = np.ascontiguousarray(arr[keep])
    o2 = np.concatenate([[0], np.cumsum(lens)]).astype("<u8")
    return dict(tables=t, runs=[_run(b2, o2, capi.CI_OPTS)], n_groups=n_cu * 128)


# ------------------------------------------------------------------ tpr: THM_HIT_GL, THM_TPR_ROUNDS
TPR_COPIES = (2, 31, 32, 33)
TPR_OPTS = dict(capi.CI_OPTS, min_aln_score_percent=0.5)


def tpr_workload():
    """dirty reads over multi-exon transcripts and the contig, and reads from planted families of 2, 31, 32 and 33 copies
    with one substitution five bases from the end: one SMEM with that many occurrences and a right side for the DP"""
    t = planted_reference(TPR_COPIES, n_genes=20, gene_region=200000, seed=0x747072)
    rng = np.random.default_rng(31)
    bases, off, _ = synth.simulate_reads(t, 3000, 91, sub_rate=0.03, indel_rate=0.008, intronic_frac=0.3, stream=701)
    reads = [bases[int(off[i]): int(off[i + 1])] for i in range(3000)]
    for f, fam in enumerate(t["_fam"]):
        for j in range(24):
            s = int(rng.integers(0, FAM_LEN - 91 + 1))
            r = fam[s: s + 91].copy()
            r[85] = _ACGT[(int(np.nonzero(_ACGT == r[85])[0][0]) + 1 + j % 3) % 4]
            if j % 4 == 3:
                r = refdata.revcomp(r)
            reads.insert(int(rng.integers(0, len(reads) + 1)), r)
    b2, o2 = refdata.pack_reads(reads)
    return dict(tables=t, runs=[_run(b2, o2, TPR_OPTS, smem_k=20)])


# ------------------------------------------------------------------ minw: THM_EXT_MINW, THM_EXT_MINW_CPL3, THM_EXT_MINW_WIDE
MINW_SHAPES = {"minw12": ((61, 31), (91, 61)), "minw34": ((120, 90), (157, 127))}  # (read length, band) under the CI options


def cells_per_lane(bw):
    return (2 * bw + 1 + 63) // 64


def minw_workload(name):
    t = synth.synth_reference(length=400000, n_genes=40)
    runs = []
    for L, bw in MINW_SHAPES[name]:
        assert L - 30 == bw
        bases, off, _ = synth.simulate_reads(t, 2000, L, sub_rate=0.03, indel_rate=0.006, intronic_frac=0.25, stream=40 + L)
        runs.append(_run(bases, off, capi.CI_OPTS))
    return dict(tables=t, runs=runs)


# ------------------------------------------------------------------ team_div: THM_TEAM_DIV_PER_CU
def team_div_workload():
    """the heavy fixture of test_gpu_align.py: reads from an 8000-copy family (hundreds to thousands of hits each)
    among ordinary reads"""
    t, pos = synth.heavy_repeat_reference(length=6_000_000, copies=8000, divergence=0.01)
    rng = np.random.default_rng(3)
    starts = pos[rng.integers(0, len(pos), 160)] + rng.integers(0, 300 - 91, 160)
    hb, ho = synth.reads_from_positions(t, starts, 91, sub_rate=0.02, stream=12)
    lb, lo, _ = synth.simulate_reads(t, 1500, 91, sub_rate=0.01, indel_rate=0.001, intronic_frac=0.3, stream=13)
    reads = [lb[int(lo[i]): int(lo[i + 1])] for i in range(1500)]
    for i in range(160):
        reads.insert(int(rng.integers(0, len(reads) + 1)), hb[int(ho[i]): int(ho[i + 1])])
    b2, o2 = refdata.pack_reads(reads)
    return dict(tables=t, runs=[_run(b2, o2, capi.CI_OPTS, smem_k=20)])


# ------------------------------------------------------------------ swg: THM_SWG_BPC
# (bw_lo, bw_hi, max_len, n).  The knob caps the grid at n_cu * THM_SWG_BPC workgroups of four waves, a wave per problem:
# it changes a launch only where n / 4 exceeds the smaller cap.  4200 problems: 1050 workgroups, beyond the default's 4 per CU
# on 256 CUs, so 1, 4 and 8 per CU are three different grids; 1200 any-width problems: 300 workgroups, capped at 1 per CU
# (waves then reuse their scratch slice); at 8 that set's grid is the default's, one slice per problem's wave
SWG_SETS = ((0, 31, 100, 4200), (32, 63, 150, 4200), (128, 200, 260, 1200))


def swg_workload():
    t = refdata.load_reference(os.path.join(_DATA, "test_ref.fasta"), os.path.join(_DATA, "test_ref.gtf"))
    sets = []
    for bw_lo, bw_hi, max_len, n in SWG_SETS:
        rng = np.random.default_rng(bw_lo * 1000 + bw_hi + 7)
        sets.append(swg_fuzz_problems(rng, n, max_len, bw_lo, bw_hi) + (bw_hi,))
    return dict(tables=t, runs=[], swg=sets)


def build(name, n_cu=N_CU_DEFAULT):
    if name == "fill":
        return fill_workload()
    if name == "compact":
        return compact_workload(n_cu)
    if name == "tpr":
        return tpr_workload()
    if name in MINW_SHAPES:
        return minw_workload(name)
    if name == "team_div":
        return team_div_workload()
    if name == "swg":
        return swg_workload()
    raise ValueError("unknown workload " + name)


# ------------------------------------------------------------------ one device run (child and parent alike)
def run_workload(w, ix, tpr=None, rounds=0):
    """every run of workload `w` on index `ix`; returns the dict of arrays that knob_child.py saves ("knobs": the 16
    words of thm_debug_knobs, see capi.knobs_dict)"""
    out = {}
    for i, r in enumerate(w["runs"]):
        a = capi.Aligner(ix, r["opts"])
        a.debug_set_flags(tpr=tpr, rounds=rounds)
        out.setdefault("knobs", a.debug_knobs())
        if r["smem_k"] is not None:
            out["smem_off%d" % i], out["smems%d" % i] = a.smems_batch(r["bases"], r["off"], r["smem_k"])
        for rep, batch in (("a", (r["bases"], r["off"])), ("b", r["second"])):
            if batch is None:
                continue
            a.reset_counters()
            g = a.align_batch(batch[0], batch[1])
            key = "%d%s" % (i, rep)
            out["off" + key], out["alns" + key], out["ops" + key] = g.offsets, g.alns, g.ops
            out["status" + key] = g.status if g.status is not None else np.zeros(g.n_reads, "<i4")
            out["n_failed" + key] = np.array([g.n_failed], "<u8")
            out["counters" + key] = a.counters()
            out["tpr_stats" + key] = a.debug_tpr_stats()
        a.close()
    if "swg" in w:
        a = capi.Aligner(ix, dict(capi.DEFAULT_OPTS, min_seed_len=3, min_aln_score=0))
        out["knobs"] = a.debug_knobs()
        for i, (xb, xo, yb, yo, bw, xd, max_bw) in enumerate(w["swg"]):
            a.reset_counters()
            out["swg_alns%d" % i], out["swg_ops%d" % i] = a.swg_extend_batch(xb, xo, yb, yo, bw, xd, max_bw)
            out["swg_counters%d" % i] = a.counters()
        a.close()
    return out


def device_n_cu():
    """compute units of device 0, from the knob report of a throw-away aligner on the smallest index"""
    t = refdata.load_reference(os.path.join(_DATA, "test_ref.fasta"), os.path.join(_DATA, "test_ref.gtf"))
    ix = capi.Index(t)
    a = capi.Aligner(ix, capi.DEFAULT_OPTS)
    n_cu = capi.knobs_dict(a.debug_knobs())["n_cu"]
    a.close()
    ix.close()
    return n_cu
