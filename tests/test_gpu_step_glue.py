"""-m gpu: what runs between the big kernels of a batch (pipeline.hip) against the oracle, at both coordinate widths.

  - the run's first launch zeroes every control word (list counts, cursors, fault words, the queue words of the seed and
    of the extend stage) and the statuses, and takes the counter snapshot a replay restores;
  - the hit-count scan is finished by plan_pack_kernel (tiles of SCAN_TILE = 2048 reads), the two output offsets come
    from one two-array scan;
  - the waves' counter rows are reduced by several workgroups that leave the rows zeroed for the next run.

The batches come from a planted reference (knob_common.planted_reference): random reads have no alignment, ordinary reads
one, reads from a family of c copies c of them; the family of 40 copies puts its reads over the team threshold of a
small batch (TEAM_MIN_HITS = 32).  The oracle runs once per batch; both widths share its result."""
import numpy as np
import pytest

from thermite_amd import capi, refdata, synth

import knob_common as kc
from gpu_common import COMPACT_HEAVY_N, World, assert_batch_equal, assert_counters_match, check_align, check_smems

pytestmark = pytest.mark.gpu

SCAN_TILE = 2048       # launch.h
TEAM_MIN_HITS = 32     # launch.h
COPIES = (2, 8, 9, 3, 40)
F9, F40 = 2, 4         # families of more than COMPACT_HEAVY_N alignments / over the team threshold
WIDTHS = pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def tables():
    return _once("tables", lambda: kc.planted_reference(COPIES, n_genes=12, gene_region=120000, seed=0x676C7565))


def n_cu():
    return _once("n_cu", kc.device_n_cu)


def world(wide):
    return _once(("world", wide), lambda: World(tables(), wide))


def fam_read(rng, f, L=91):
    fam = tables()["_fam"][f]
    s = int(rng.integers(0, kc.FAM_LEN - L + 1))
    r = fam[s: s + L]
    return refdata.revcomp(r) if rng.random() < 0.5 else r.copy()


def random_read(rng, L=91):
    return _ACGT[rng.integers(0, 4, L)]


def mixed_reads(n, seed, team=False):
    """kinds by batch position i % 7: 0, 3, 6 ordinary reads (transcripts and contig), 1 random (no alignment), 2 / 4 / 5
    reads from the families of 2 / 8 / 9 copies; team: every 50th read from the family of 40 copies"""
    t = tables()
    rng = np.random.default_rng(seed)
    bases, off, _ = synth.simulate_reads(t, max(n, 1), 91, sub_rate=0.01, indel_rate=0.001, intronic_frac=0.3, stream=seed)
    reads = [bases[int(off[i]): int(off[i + 1])] for i in range(n)]
    for i in range(n):
        k = i % 7
        if k == 1:
            reads[i] = random_read(rng)
        elif k in (2, 4, 5):
            reads[i] = fam_read(rng, {2: 0, 4: 1, 5: F9}[k])
        if team and i % 50 == 17:
            reads[i] = fam_read(rng, F40)
    return reads


def oracle(key, bases, off, opts=capi.CI_OPTS):
    def make():
        r = world(False).oix.align_batch(bases, off, opts, n_threads=16)
        assert r.counters[15] == 0, "oracle saw reads where the reference would panic"
        return r
    return _once(("oracle", key), make)


# ------------------------------------------------------------------ scan boundaries
def boundary_batch(n, swap):
    """n mixed reads; at every tile boundary b of the scans (multiples of SCAN_TILE) a read without alignments in slot
    b - 1 and one with more than COMPACT_HEAVY_N in slot b -- the other way round at every second boundary, and at
    every boundary the other way round again with swap.  A batch that ends at b - 1 ends with that read."""
    def make():
        rng = np.random.default_rng(1000 + n)
        reads = mixed_reads(n, 900 + n)
        zero_slots, heavy_slots = [], []
        for j, b in enumerate(range(SCAN_TILE, n + 2, SCAN_TILE)):
            last_is_zero = (j % 2 == 0) != swap
            for slot, is_zero in ((b - 1, last_is_zero), (b, not last_is_zero)):
                if slot < n:
                    (zero_slots if is_zero else heavy_slots).append(slot)
        if n == 1:
            (zero_slots if swap else heavy_slots).append(0)
        for s in zero_slots:
            reads[s] = random_read(rng)
        for s in heavy_slots:
            reads[s] = fam_read(rng, F9)
        bases, off = refdata.pack_reads(reads) if n else (np.zeros(0, np.uint8), np.zeros(1, "<u8"))
        return bases, off, zero_slots, heavy_slots
    return _once(("boundary", n, swap), make)


@WIDTHS
@pytest.mark.parametrize("n,swap", [(0, False), (1, False), (1, True), (2047, False), (2047, True), (2048, False), (2048, True),
                                    (2049, False), (2049, True), (4097, False), (4097, True)])
def test_scan_tile_boundaries(n, swap, wide):
    bases, off, zero_slots, heavy_slots = boundary_batch(n, swap)
    ref = oracle(("boundary", n, swap), bases, off)
    n_alns = np.diff(ref.offsets.astype(np.int64))
    assert all(n_alns[s] == 0 for s in zero_slots) and all(n_alns[s] > COMPACT_HEAVY_N for s in heavy_slots)
    if n >= SCAN_TILE - 1:
        assert (n_alns == 0).sum() > 100 and (n_alns == 1).sum() > 100 and (n_alns > COMPACT_HEAVY_N).sum() > 100
    assert n < SCAN_TILE or len(zero_slots) + len(heavy_slots) >= 1
    w = world(wide)
    check_align(w, bases, off, capi.CI_OPTS, ref=ref)
    check_smems(w, bases, off, 20)   # the seed-only entry finishes the same scan with its own add phase


# ------------------------------------------------------------------ counter rows
def smem_hits(bases, off):
    """seed hits per read under the CI options' seed length, from the oracle"""
    return np.diff(world(False).oix.all_smems(bases, off, 20).offsets.astype(np.int64))


def counter_batches():
    def make():
        n_big = 3 * n_cu() * 128 + 87   # every wave of the main grid takes work
        out = []
        for key, reads in (("big", mixed_reads(n_big, 11)), ("three", mixed_reads(3, 12)),
                           ("team", mixed_reads(3000, 13, team=True)), ("plain", mixed_reads(3000, 14))):
            bases, off = refdata.pack_reads(reads)
            if key == "plain":   # an ordinary read may come from the planted region: none may reach the team threshold
                rng = np.random.default_rng(15)
                for i in np.nonzero(smem_hits(bases, off) >= TEAM_MIN_HITS)[0]:
                    reads[i] = fam_read(rng, 0)
                bases, off = refdata.pack_reads(reads)
            out.append((key, bases, off, oracle(("counters", key), bases, off)))
        return out
    return _once("counter_batches", make)


@WIDTHS
def test_counter_rows_stay_clean(wide):
    """One aligner: a batch that leaves a row for every wave of the grid, then one of three reads (a stale row would be
    counted again), then one with reads on the team list, then one without.  Counters are the oracle's running sums;
    reset_counters starts them again."""
    batches = counter_batches()
    w = world(wide)
    team = batches[2]
    hits = smem_hits(team[1], team[2])
    on_team = int((hits >= TEAM_MIN_HITS).sum())
    assert 20 <= on_team <= 2 * n_cu(), on_team      # the team kernel takes them (team_limit, pipeline.hip)
    assert hits.sum() // (22 * n_cu()) < TEAM_MIN_HITS  # ... at the lowest threshold
    assert int((smem_hits(batches[3][1], batches[3][2]) >= TEAM_MIN_HITS).sum()) == 0
    a = w.aligner(capi.CI_OPTS)
    a.reset_counters()
    total = np.zeros(capi.N_COUNTERS, "<u8")
    for i, (key, bases, off, ref) in enumerate(batches):
        if i == 2:
            a.reset_counters()
            total[:] = 0
        g = a.align_batch(bases, off)
        assert g.n_failed == 0
        assert_batch_equal(g, ref)
        total += ref.counters
        assert_counters_match(a.counters(), total, key)
    a.close()


def slow_batch():
    """2000 mixed reads of 91 bases with 24 reads of 300 - 1000 bases among them: under the CI options (band = L - 30) the
    long ones are the slow class, which the any-width launch takes"""
    def make():
        t = tables()
        rng = np.random.default_rng(31)
        reads = mixed_reads(2000, 16)
        for j, L in enumerate([300, 333, 450, 512, 640, 777, 1000, 1000]):
            lb, lo, _ = synth.simulate_reads(t, 3, L, sub_rate=0.02, indel_rate=0.004, intronic_frac=0.5, stream=80 + j)
            for i in range(3):
                reads.insert(int(rng.integers(0, len(reads) + 1)), lb[int(lo[i]): int(lo[i + 1])])
        bases, off = refdata.pack_reads(reads)
        return bases, off, oracle(("counters", "slow"), bases, off)
    return _once("slow_batch", make)


@WIDTHS
def test_counter_rows_across_launch_mixes(wide):
    """One aligner, consecutive batches whose launches differ, so that the sections of the counter rows (main | team | slow |
    problem-parallel path | finisher) come and go from run to run: the finisher without team reads, team reads, the slow
    class, the problem-parallel path (no finisher), and three reads on the default path again.  Records and op bytes are
    the oracle's after every run and the counters its running sums: a row written outside its section, or left unreduced,
    is a wrong sum in the following run."""
    by_key = {key: (bases, off, ref) for key, bases, off, ref in counter_batches()}
    by_key["slow"] = slow_batch()
    lens = np.diff(by_key["slow"][1].astype(np.int64))
    assert (lens > 255).sum() == 24 and (np.diff(by_key["slow"][2].offsets.astype(np.int64))[lens > 255] > 0).sum() >= 12
    a = world(wide).aligner(capi.CI_OPTS)
    a.debug_set_flags(tpr=False)
    a.reset_counters()
    total = np.zeros(capi.N_COUNTERS, "<u8")
    for step, (key, tpr) in enumerate([("plain", False), ("team", False), ("slow", False), ("team", True), ("three", False)]):
        bases, off, ref = by_key[key]
        a.debug_set_flags(tpr=tpr)
        g = a.align_batch(bases, off)
        assert g.n_failed == 0
        assert_batch_equal(g, ref)
        total += ref.counters
        assert_counters_match(a.counters(), total, (step, key, tpr))
        # the launches that make the step what it is did run
        assert int(a.debug_knobs()[13]) == int(tpr)
        fin = a.debug_smem_finish_stats()   # (of three reads none may have one of the finisher's shapes)
        assert sum(fin) == 0 if tpr else (fin[0] + fin[2] > 0 or key == "three"), (step, fin)
        if tpr:
            assert a.debug_tpr_stats()[16] > 0   # DP records the rounds asked for
    a.close()


# ------------------------------------------------------------------ replay
def replay_batch():
    def make():
        bases, off = refdata.pack_reads(mixed_reads(3000, 21))
        return bases, off, oracle("replay", bases, off)
    return _once("replay", make)


@WIDTHS
@pytest.mark.parametrize("caps", [dict(smem_cap=512), dict(ops_cap=8192)], ids=["smem_pool", "op_pool"])
def test_replay_on_the_second_run(caps, wide):
    """the second run of an aligner overflows a pool: the replay gives the same records and counts once"""
    bases, off, ref = replay_batch()
    a = world(wide).aligner(capi.CI_OPTS)
    a.reset_counters()
    assert_batch_equal(a.align_batch(bases, off), ref)
    assert_counters_match(a.counters(), ref.counters, "first run")
    before = a.debug_set_pool_caps(**caps)
    g = a.align_batch(bases, off)
    assert a.debug_set_pool_caps() > before, "the small pool did not overflow: %r" % (caps,)
    assert_batch_equal(g, ref)
    assert_counters_match(a.counters(), ref.counters * np.uint64(2), "after the replay")
    # and a run after the replay, with the heuristic pool sizes again
    assert_batch_equal(a.align_batch(bases, off), ref)
    assert_counters_match(a.counters(), ref.counters * np.uint64(3), "third run")
    a.close()


# ------------------------------------------------------------------ seed-only entry between two runs
@WIDTHS
def test_seed_only_entry_between_runs(wide):
    bases, off, ref = replay_batch()
    w = world(wide)
    mems = _once("replay_mems", lambda: w.oix.all_smems(bases, off, 15))
    a = w.aligner(capi.CI_OPTS)
    assert_batch_equal(a.align_batch(bases, off), ref)
    g_off, g_mems = a.smems_batch(bases, off, 15)
    assert np.array_equal(g_off, mems.offsets)
    for f in ("ref_idx", "query_idx", "len"):
        assert np.array_equal(g_mems[f], mems.mems[f]), f
    a.reset_counters()
    g = a.align_batch(bases, off)
    assert g.n_failed == 0
    assert_batch_equal(g, ref)
    assert_counters_match(a.counters(), ref.counters, "run after the seed-only call")
    a.close()


# ------------------------------------------------------------------ the two stages' queue words
@WIDTHS
def test_queue_words_of_both_stages(wide):
    """91-base reads, reads over 255 bases (their SMEM selection takes its reads from the seed stage's queue words) and the
    slow class (band = L - 30 beyond +-127: the any-width kernel, which takes its reads from the extend stage's) in one
    batch, under the reference's chr21 flags"""
    def make():
        t = synth.synth_reference(length=400000, n_genes=40)
        rng = np.random.default_rng(41)
        bases, off, _ = synth.simulate_reads(t, 400, 91, sub_rate=0.01, indel_rate=0.001, intronic_frac=0.2, stream=51)
        reads = [bases[off[i]: off[i + 1]] for i in range(400)]
        for j, L in enumerate([300, 333, 450, 512, 640, 777, 1000, 1000]):
            lb, lo, _ = synth.simulate_reads(t, 3, L, sub_rate=0.02, indel_rate=0.004, intronic_frac=0.5, stream=60 + j)
            for i in range(3):
                reads.insert(int(rng.integers(0, len(reads) + 1)), lb[lo[i]: lo[i + 1]])
        return (t,) + tuple(refdata.pack_reads(reads))
    t, bases, off = _once("queue_batch", make)
    w = _once(("queue_world", wide), lambda: World(t, wide))
    ref = _once("queue_oracle", lambda: w.oix.align_batch(bases, off, capi.CI_OPTS, n_threads=16))
    lens = np.diff(off.astype(np.int64))
    n_alns = np.diff(ref.offsets.astype(np.int64))
    assert (lens > 255).sum() == 24 and (n_alns[lens > 255] > 0).sum() >= 12 and (n_alns[lens == 91] > 0).sum() > 300
    check_smems(w, bases, off, 20)
    check_align(w, bases, off, capi.CI_OPTS, ref=ref)
