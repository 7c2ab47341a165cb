"""Batches of tests/test_gpu_compact_tiles.py, shared with tests/test_compact_copy_host.py, which pins with the oracle
alone what they reach.  The compact kernel (kernels_compact.hip) takes a workgroup per tile of COMPACT_TILE consecutive
reads: a thread per read writes one descriptor per alignment, then a 16-lane group per alignment copies the record and
the op streams as aligned dwords with single bytes at either end.

The reference is knob_common.planted_reference with families of 2, 8, 9 and 3 copies: random reads have no alignment,
ordinary reads one, a read from inside a family as many as the family has copies."""
import numpy as np

from thermite_amd import capi, refdata, synth

import knob_common as kc

COMPACT_TILE = 256     # kernels_compact.hip
COPIES = (2, 8, 9, 3)
F2, F8, F9, F3 = 0, 1, 2, 3
BOUNDARY_NS = (1, COMPACT_TILE - 1, COMPACT_TILE, COMPACT_TILE + 1, 2 * COMPACT_TILE + 1)
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def tables():
    return once("tables", lambda: kc.planted_reference(COPIES, n_genes=12, gene_region=120000, seed=0x74696C65))


def fam_read(rng, f, L=91):
    fam = tables()["_fam"][f]
    s = int(rng.integers(0, kc.FAM_LEN - L + 1))
    r = fam[s: s + L]
    return refdata.revcomp(r) if rng.random() < 0.5 else r.copy()


def random_read(rng, L=91):
    return _ACGT[rng.integers(0, 4, L)]


def mixed_reads(n, seed, ragged=False):
    """kinds by batch position i % 7: 0, 3 ordinary reads (transcripts and contig), 1 random (no alignment), 2 / 4 / 5 / 6
    reads from the families of 2 / 8 / 9 / 3 copies; 91 bases, or ragged: 60..120"""
    rng = np.random.default_rng(seed)
    bases, off, _ = synth.simulate_reads(tables(), max(n, 1), 120, sub_rate=0.01, indel_rate=0.001, intronic_frac=0.4, stream=seed)
    reads = []
    for i in range(n):
        L = int(rng.integers(60, 121)) if ragged else 91
        k = i % 7
        if k == 1:
            reads.append(random_read(rng, L))
        elif k in (2, 4, 5, 6):
            reads.append(fam_read(rng, {2: F2, 4: F8, 5: F9, 6: F3}[k], L))
        else:
            reads.append(bases[int(off[i]): int(off[i]) + L])
    return reads


def boundary_batch(n, swap):
    """n mixed reads; the first without an alignment, the last from the family of 9 copies (more than COMPACT_HEAVY_N
    alignments).  At every multiple b of COMPACT_TILE a read without alignments in slot b - 1 and one of the 9-copy family
    in slot b -- the other way round at every second boundary, and at every boundary the other way round again with
    swap; where such a slot is the batch's first or last read, the boundary decides.  n = 1: that one read has no alignment,
    with swap it has nine.  Returns bases, off, zero_slots, heavy_slots."""
    def make():
        rng = np.random.default_rng(2000 + n)
        reads = mixed_reads(n, 1900 + n)
        kind = {}
        if n > 1:
            kind[0], kind[n - 1] = True, False
        else:
            kind[0] = not swap
        for j, b in enumerate(range(COMPACT_TILE, n + 2, COMPACT_TILE)):
            last_is_zero = (j % 2 == 0) != swap
            for slot, is_zero in ((b - 1, last_is_zero), (b, not last_is_zero)):
                if slot < n:
                    kind[slot] = is_zero
        for s, is_zero in kind.items():
            reads[s] = random_read(rng) if is_zero else fam_read(rng, F9)
        bases, off = refdata.pack_reads(reads)
        return bases, off, sorted(s for s in kind if kind[s]), sorted(s for s in kind if not kind[s])
    return once(("boundary", n, swap), make)


N_LONG = 10  # reads of 250, of 1000 and of 1100 bases in the ragged batch


def ragged_batch():
    """about 3 tiles of reads of 60..120 bases, and among them N_LONG reads each of 250, 1000 and 1100 bases (the last
    two are the slow class under the CI options: band = L - 30), half of them from transcripts: exonic alignments of
    multi-exon transcripts carry a genome and a transcript op stream"""
    def make():
        t = tables()
        rng = np.random.default_rng(51)
        reads = mixed_reads(3 * COMPACT_TILE - 11, 52, ragged=True)
        for j, L in enumerate((250, 1000, 1100)):
            lb, lo, _ = synth.simulate_reads(t, N_LONG, L, sub_rate=0.02, indel_rate=0.004, intronic_frac=0.5, stream=90 + j)
            for i in range(N_LONG):
                reads.insert(int(rng.integers(0, len(reads) + 1)), lb[int(lo[i]): int(lo[i + 1])])
        return refdata.pack_reads(reads)
    return once("ragged", make)


def empty_batch():
    """two tiles of random reads: no read has an alignment"""
    def make():
        rng = np.random.default_rng(61)
        return refdata.pack_reads([random_read(rng) for _ in range(2 * COMPACT_TILE)])
    return once("empty", make)


def all_batches():
    """(key, bases, off) of every batch of the GPU test"""
    out = [(("boundary", n, swap),) + boundary_batch(n, swap)[:2] for n in BOUNDARY_NS for swap in (False, True)]
    out.append((("ragged",),) + tuple(ragged_batch()))
    out.append((("empty",),) + tuple(empty_batch()))
    return out


def oracle(oix, key, bases, off, opts=capi.CI_OPTS):
    def make():
        r = oix.align_batch(bases, off, opts, n_threads=16)
        assert r.counters[15] == 0, "oracle saw reads where the reference would panic"
        return r
    return once(("oracle", key), make)
