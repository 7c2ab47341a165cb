"""Worlds, read sets and the case table of the tests at the limits of AlignOpts (test_opts_limits_host.py pins the read
sets with the oracle alone, test_gpu_opts_limits.py compares the device with it).

thm_align_opts holds a u64 multimap_score_range, an i32 min_aln_score, a u64 min_seed_len, a float and an int used as a
bool; the rest of the suite stays inside min_seed_len 3..40, a percentage of 0.0..0.9, min_aln_score 0 / 20 / 30 and a
range of 0..6.  The cases here are the values at which the arithmetic of align_read (reference src/aligner.rs:130-179)
changes its behaviour -- all of them defined in the reference: neither `read.len() + range` nor
`max_aln_score - (range as i32)` overflows for any of them.

  rep: 40 copies of a 300-mer, 3 % diverged.  A read from one copy with an inserted or a deleted base aligns to most of
       the others as well, each time with a gap; whether the later ones are found depends on the band that is left after
       the first accepted alignment -- min(band, L + range - score), in usize arithmetic with the untruncated range.
  syn: an ordinary synthetic transcriptome, for the score thresholds and the seed lengths."""
import numpy as np

from oracle import pyoracle as orc
from thermite_amd import refdata, synth

L = 91
I32_MAX = 2 ** 31 - 1

# ------------------------------------------------------------------ rep: multimappers that need a band
REP_OPTS = dict(min_seed_len=20, min_aln_score_percent=0.66, min_aln_score=30, multimap_score_range=1, intron_mode=True)
# (value, what it is)
RANGES = [
    (91, "L"),
    (1000, "1000"),
    (I32_MAX - 91, "i32max-L"),       # the largest range for which L + range fits an int at L = 91
    (I32_MAX - 90, "i32max-L+1"),     # the first for which it does not
    (I32_MAX, "i32max"),              # "keep every multimapper"
    (2 ** 32 - 1, "u32max"),          # as i32: -1 -- the final retain asks for score >= max + 1: no read keeps an alignment
    (2 ** 32, "2p32"),                # as i32: 0, low 32 bits 0; the band never narrows
    (2 ** 32 + 1, "2p32+1"),
    (2 ** 32 + 6, "2p32+6"),
    (2 ** 63, "2p63"),
]
RANGE_IDS = [name for _, name in RANGES]


def rep_tables():
    """(tables, start positions of the copies)"""
    return synth.heavy_repeat_reference(length=300000, copies=40, unit_len=300, divergence=0.03, n_genes=8)


def rep_reads(t, pos):
    """240 reads of 91 bases: 40 reads from the copies, six variants of each with one inserted (even variants: a copy of
    the base in front) or one deleted base at a position of 25..65"""
    bases, off = synth.reads_from_positions(t, pos[:40] + 40, 93, sub_rate=0.01, stream=3)
    rng = np.random.default_rng(9)
    reads = []
    for i in range(40):
        r = bases[int(off[i]): int(off[i + 1])]
        for v in range(6):
            p = int(rng.integers(25, 66))
            e = np.concatenate([r[:p], r[p - 1: p], r[p:]]) if v % 2 == 0 else np.concatenate([r[:p], r[p + 1:]])
            reads.append(np.ascontiguousarray(e[:L]))
    return refdata.pack_reads(reads)


def rep_opts(rng_value):
    return dict(REP_OPTS, multimap_score_range=rng_value)


# ------------------------------------------------------------------ syn: score thresholds and seed lengths
SYN_OPTS = dict(min_seed_len=20, min_aln_score_percent=0.66, min_aln_score=30, multimap_score_range=1, intron_mode=True)
N_SYN, N_SEED = 1500, 300


def syn_tables():
    return synth.synth_reference(length=400000, n_genes=40)


def syn_reads(t):
    bases, off, _ = synth.simulate_reads(t, N_SYN, L, sub_rate=0.004, indel_rate=0.0005, intronic_frac=0.25, stream=502)
    return bases, off


def first_reads(bases, off, n):
    return bases[: int(off[n])], off[: n + 1]


def cut_reads(bases, off, seed=77):
    """the same reads cut to random lengths 0..L (both ends of the interval occur)"""
    rng = np.random.default_rng(seed)
    n = len(off) - 1
    lens = rng.integers(0, L + 1, n)
    lens[:4] = (0, L, 1, L - 1)
    return refdata.pack_reads([bases[int(off[i]): int(off[i]) + int(lens[i])] for i in range(n)])


# name -> (options, reads: "all" | "cut" | "first")
SCORE_CASES = {
    "pct1": (dict(SYN_OPTS, min_aln_score_percent=1.0), "all"),          # band and X-drop 0 from the start
    "pct1_cut": (dict(SYN_OPTS, min_aln_score_percent=1.0), "cut"),
    "min200": (dict(SYN_OPTS, min_aln_score=200), "all"),               # above L: every hit is extended, none accepted
    "min_i32max": (dict(SYN_OPTS, min_aln_score=I32_MAX), "all"),
    "pct0_min-7": (dict(SYN_OPTS, min_aln_score_percent=0.0, min_aln_score=-7), "first"),    # max(0, -7) = 0: band L
    "pct0_min_i32min": (dict(SYN_OPTS, min_aln_score_percent=0.0, min_aln_score=-2 ** 31), "first"),
}
SEED_LENS = [1, 2, L, L + 1, 65535]
SEED_LENS_REFUSED = [0, 65536]


def syn_case_reads(bases, off, which):
    if which == "all":
        return bases, off
    if which == "cut":
        return cut_reads(bases, off)
    return first_reads(bases, off, N_SEED)


def seed_opts(k):
    return dict(SYN_OPTS, min_seed_len=k)


# ------------------------------------------------------------------ set_opts between runs
# The sequence's base options: the flags of the reference's CI runs (-k20 --intron-mode) at the default percentage --
# band 31 at L = 91, one DP cell per lane of the extend kernel (2 * 31 + 1 <= 64).
BASE = dict(min_seed_len=20, min_aln_score_percent=0.66, min_aln_score=30, multimap_score_range=1, intron_mode=True)
PCT03 = dict(BASE, min_aln_score_percent=0.3)   # max(27, 30) = 30: band 61, two cells per lane
# (name, options, read set).  An aligner has one index, so both read sets of the sequence are for the rep world: "rep",
# and "sim", reads simulated from rep's own genes and contig with the parameters of the syn reads.
SEQUENCE = [
    ("base", BASE, "rep"),
    ("pct03", PCT03, "sim"),
    ("pct0_min0", dict(BASE, min_aln_score_percent=0.0, min_aln_score=0), "rep"),   # band 91, three cells per lane
    ("range_i32max", dict(BASE, multimap_score_range=I32_MAX), "rep"),
    ("pct1", dict(BASE, min_aln_score_percent=1.0), "sim"),                         # band 0
    ("seed12", dict(BASE, min_seed_len=12), "rep"),
    ("no_intron", dict(BASE, intron_mode=False), "sim"),
    ("ci_flags", dict(BASE, min_aln_score_percent=0.0), "sim"),                     # capi.CI_OPTS: -k20 -s0 --intron-mode
    ("base_again", BASE, "rep"),
]
N_SIM = 600
REPLAY_CAPS = dict(smem_cap=300, cand_cap=16, ops_cap=4096)     # pools so small that a run of either read set replays


def sim_reads(t):
    bases, off, _ = synth.simulate_reads(t, N_SIM, L, sub_rate=0.004, indel_rate=0.0005, intronic_frac=0.25, stream=502)
    return bases, off


def band_at_L(opts):
    """align_read's initial band for a read of L bases, src/aligner.rs:130-138"""
    ms = max(int(np.float32(opts["min_aln_score_percent"]) * np.float32(L)), opts["min_aln_score"])
    return max(L - ms, 0) if ms >= 0 else 0   # (`as usize` of a negative score wraps: the saturating_sub gives 0)


def n_gapped(res, i):
    """alignments of read i of an oracle (or device) result whose genomic op stream holds an Ins or a Del"""
    n = 0
    for j in range(int(res.offsets[i]), int(res.offsets[i + 1])):
        a = res.alns[j]
        ops = orc.decode_ops(res.ops[int(a["ops_off"]): int(a["ops_off"]) + int(a["ops_len"])])
        n += any(o in ("Ins", "Del") for o in ops)
    return n


def results_equal(a, b):
    return np.array_equal(a.offsets, b.offsets) and np.array_equal(a.alns, b.alns) and np.array_equal(a.ops, b.ops)
