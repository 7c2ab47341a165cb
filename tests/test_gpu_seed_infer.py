"""-m gpu: seed probes decided from the k-mer table entry and a neighbouring match (kernels_seed.hip).

A probe behind position 0 is told the end of a match further left in its read.  Where that match covers the probe's
kt-mer and the table holds a single suffix for it, the probe returns without reading the suffix array or the text, and
a probe stores its interval only where an SMEM can start.  Bit 2 of thm_debug_set_flags turns both off (bit 4: on again), bit 3 makes
the seed kernels count their probes (thm_debug_seed_stats: decided from the table entry alone, run in full).

Every case goes through gpu_common.check_smems and check_align against the oracle, at 32- and 64-bit coordinates, with
the shortcut on and off, and asserts from the counts that it reached the branch it names: decided > 0 where the shortcut
must fire, == 0 where it cannot (and always with the bit off).  The probed positions do not depend on the shortcut, so
decided + full with it equals full without it.

One text of 36 kilobases in two contigs (an N run, a 60-base stretch that occurs twice), indexed with THM_KT = 8; the
cases hold at most a few hundred reads each."""
import os

import numpy as np
import pytest

from thermite_amd import capi, refdata, synth

from gpu_common import World, check_align, check_smems

pytestmark = pytest.mark.gpu

KT = 8
ACGT = np.frombuffer(b"ACGT", np.uint8)
MAIN_LEN, SECOND_LEN = 30000, 6000
DUP_A, DUP_B, DUP_LEN = 5000, 9000, 60       # main[DUP_B : DUP_B + 60] is a copy of main[DUP_A : DUP_A + 60]
N_RUN = (15000, 15200)                       # main[15000:15200] is N
SHORT_READ_MAX = 255                         # launch.h
OPTS = dict(capi.CI_OPTS)

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _other(*avoid):
    return int([b for b in ACGT if int(b) not in [int(a) for a in avoid]][0])


def _make_tables():
    rng = np.random.Generator(np.random.PCG64(0x5EED1F))
    main = ACGT[rng.integers(0, 4, MAIN_LEN)].copy()
    main[DUP_B: DUP_B + DUP_LEN] = main[DUP_A: DUP_A + DUP_LEN]
    main[DUP_B - 1] = _other(main[DUP_A - 1])               # the copies differ in front ...
    main[DUP_B + DUP_LEN] = _other(main[DUP_A + DUP_LEN])   # ... and behind
    main[N_RUN[0]: N_RUN[1]] = ord("N")
    second = ACGT[rng.integers(0, 4, SECOND_LEN)].copy()
    genes, txs = synth.synth_annotation(rng, "main", MAIN_LEN, 100, 4)
    t = refdata.build_tables([("main", main), ("second", second)], genes, txs)
    t["_main"], t["_second"] = main, second
    return t


def tables():
    return _once("tables", _make_tables)


def world(wide):
    def make():
        old = os.environ.get("THM_KT")
        os.environ["THM_KT"] = str(KT)   # read when the index is created
        try:
            return World(tables(), wide)
        finally:
            if old is None:
                del os.environ["THM_KT"]
            else:
                os.environ["THM_KT"] = old
    return _once(("world", wide), make)


class _CountingAligner(capi.Aligner):
    sink = None

    def close(self):
        if getattr(self, "h", None) and self.sink is not None:
            self.sink.append(self.debug_seed_stats())   # the aligner's one batch
        super().close()


class FlagWorld:
    """what check_smems and check_align use of a World; its aligners have the shortcut on or off, count their seed
    probes and leave the counts in .stats when the check closes them"""

    def __init__(self, w, infer):
        self.t, self.ix, self.oix = w.t, w.ix, w.oix
        self.infer = infer
        self.stats = []

    def aligner(self, opts):
        a = _CountingAligner(self.ix, opts)
        a.sink = self.stats
        a.debug_set_flags(seed_infer=self.infer, seed_stats=True)   # (check_align's own debug_set_flags keeps the two)
        return a


def sub(read, p):
    r = np.array(read, np.uint8)
    r[p] = _other(r[p])
    return r


def window(s, L, contig="_main"):
    return tables()[contig][s: s + L].copy()


# ------------------------------------------------------------------ the cases: name -> (reads, k, the shortcut must fire)
def _one_sub(L, k=20):
    reads = []
    for s in (2000, 21011):
        w = window(s, L)
        reads += [sub(w, p) for p in range(L)]
    reads.append(refdata.revcomp(sub(window(2500, L), L // 2)))
    return reads, k, True


def _two_subs():
    reads = []
    w = window(3000, 91)
    for p in range(0, 80, 3):
        for gap in (1, 7, 8, 13, 19):              # fewer than k apart: the grid points between them and k behind have end 0
            if p + gap < 91:
                reads.append(sub(sub(w, p), p + gap))
        for gap in (29, 30, 37, 50):               # more than k + 8 apart
            if p + gap < 91:
                reads.append(sub(sub(w, p), p + gap))
    return reads, 20, True


def _duplicate():
    """reads that start inside the duplicated stretch, follow one copy and have a substitution on the first base behind
    the stretch: every kt-mer the match from position 0 covers has both copies in its bucket"""
    main = tables()["_main"]
    reads = []
    for at in (DUP_A, DUP_B):
        other = DUP_B if at == DUP_A else DUP_A
        for s in range(0, 21):
            r = window(at + s, 91)
            r[DUP_LEN - s] = _other(main[at + DUP_LEN], main[other + DUP_LEN])
            reads.append(r)
    return reads, 20, False


def _contig_end():
    rng = np.random.Generator(np.random.PCG64(0xE2D))
    reads = []
    for n in (30, 40, 47, 48, 49, 60):
        tail = ACGT[rng.integers(0, 4, 91 - n)]
        reads.append(np.concatenate([window(SECOND_LEN - n, n, "_second"), tail]))   # the match stops at '$'
        reads.append(np.concatenate([window(MAIN_LEN - n, n), tail]))
        reads.append(np.concatenate([window(N_RUN[0] - n, n), tail]))                # ... at the N run
        nn = np.frombuffer(b"NN", np.uint8)
        reads.append(np.concatenate([window(N_RUN[0] - n, n), nn, tail[2:]]))        # ... two bases into it
        reads.append(refdata.revcomp(np.concatenate([tail, window(0, n, "_second")])))  # the other strand's contig end
    w = window(4000, 91)
    for p in (0, 7, 8, 33, 45, 70, 90):
        for c in (b"N", b"n", b"X", b"*", b"\x00", b"$"):
            r = w.copy()
            r[p] = c[0]
            reads.append(r)
    r = w.copy()
    r[40:44] = ord("N")
    reads.append(r)
    return reads, 20, True


def _small_k():
    w = window(6000, 40)
    return [w] + [sub(w, p) for p in range(0, 40, 3)], KT - 2, False      # k < kt: no table


def _k_is_kt():
    w = window(6500, 50)
    return [w] + [sub(w, p) for p in range(50)], KT, True


def _k40():
    w = window(7000, 140)
    return [sub(w, p) for p in range(140)] + [sub(sub(w, p), p + 45) for p in range(0, 90, 5)], 40, True  # walk-left of 6 grid points


def _long_reads():
    reads = [sub(window(2000 + 97 * i, 91), (7 * i) % 91) for i in range(40)]
    for L in (SHORT_READ_MAX, SHORT_READ_MAX + 1, 300, 1500):
        w = window(10000 + L, L)
        for p in range(17, L, 61):
            w = sub(w, p)
        reads.insert(len(reads) // 2, w)
    return reads, 20, True


def _indels():
    reads = []
    w = window(12000, 92)
    for p in range(4, 88, 3):
        reads.append(np.concatenate([w[:p], [_other(w[p - 1], w[p])], w[p: 90]]).astype(np.uint8))   # one inserted base
        reads.append(np.concatenate([w[:p], w[p + 1:]]).astype(np.uint8))                             # one deleted base
    return reads, 20, True


CASES = {
    "one_sub_L91": lambda: _one_sub(91),
    "one_sub_L29": lambda: _one_sub(29),
    "one_sub_L35": lambda: _one_sub(35),
    "two_subs": _two_subs,
    "duplicate": _duplicate,
    "contig_end": _contig_end,
    "small_k": _small_k,
    "k_is_kt": _k_is_kt,
    "k40": _k40,
    "long_reads": _long_reads,
    "indels": _indels,
}


def case(name):
    def make():
        reads, k, fires = CASES[name]()
        bases, off = refdata.pack_reads(reads)
        return bases, off, k, fires
    return _once(("case", name), make)


def oracle_alignments(name):
    """the oracle's alignments of a case: once, for both widths and both settings"""
    def make():
        bases, off, k, _ = case(name)
        return world(False).oix.align_batch(bases, off, dict(OPTS, min_seed_len=k), n_threads=8)
    return _once(("oracle", name), make)


def test_the_index_has_the_table_the_cases_assume():
    w = world(False)
    t = tables()
    main = t["_main"]
    assert np.array_equal(main[DUP_A: DUP_A + DUP_LEN], main[DUP_B: DUP_B + DUP_LEN])
    assert main[DUP_A + DUP_LEN] != main[DUP_B + DUP_LEN] and main[DUP_A - 1] != main[DUP_B - 1]
    # the reads of the duplicate case have one SMEM of two occurrences, from position 0 to the end of the stretch
    bases, off, k, _ = case("duplicate")
    r = w.oix.all_smems(bases, off, k)
    for i in range(len(off) - 1):
        m = r.mems[int(r.offsets[i]): int(r.offsets[i + 1])]
        s = i % 21
        first = m[(m["query_idx"] == 0) & (m["len"] == DUP_LEN - s)]
        assert len(first) == 2, (i, m)
    # a read longer than SHORT_READ_MAX stands among short ones
    lens = np.diff(case("long_reads")[1].astype(np.int64))
    assert (lens == SHORT_READ_MAX).any() and (lens == SHORT_READ_MAX + 1).any() and (lens == 300).any() and (lens <= 91).sum() >= 40
    for name in ("one_sub_L29", "one_sub_L35"):
        lens = np.diff(case(name)[1].astype(np.int64))
        assert ((lens - 20) % 8 != 0).all()   # npos - 1 inside a cell


@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_seed_infer(name, wide):
    bases, off, k, fires = case(name)
    opts = dict(OPTS, min_seed_len=k)
    ref = oracle_alignments(name)
    totals = {}
    for infer in (True, False):
        fw = FlagWorld(world(wide), infer)
        check_smems(fw, bases, off, k)
        check_align(fw, bases, off, opts, ref=ref)
        assert len(fw.stats) == 3, fw.stats   # smems_batch, align_batch with and without the problem-parallel path
        print(name, "wide" if wide else "narrow", "infer" if infer else "full", fw.stats)
        for decided, full in fw.stats:
            assert full > 0, fw.stats
            if infer and fires:
                assert decided > 0, fw.stats
            else:
                assert decided == 0, fw.stats
        totals[infer] = [d + f for d, f in fw.stats]
    assert totals[True] == totals[False], totals   # the same positions were probed
