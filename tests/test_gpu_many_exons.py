"""-m gpu: alignments across more introns than the register-resident extend kernels keep markers for.

Those kernels hold FAST_MAX_YCLIPS = 64 intron markers per alignment (extend_plan.h).  An alignment that needs more sets
FAULT_RETRY: the read goes on the retry list, its wave's DP counters are zeroed, and the any-width kernel redoes it
(lift_markers in extend_device.h, kernels_extend.hip).  The host arms this when the index has a transcript of more than 65 exons (pipeline.hip,
seed_hits.hip), which no other reference of the suite has.  The micro-exon reference of gpu_common has transcripts of up
to 202 exons; tests/test_many_exons_host.py pins, with the oracle alone, that its read sets have alignments on both sides
of the limit.  Every test states the path it enters as an assertion on oracle or smems_batch output, and compares
results and counters with the oracle through check_align (both extend paths; the counter comparison is the check on the
reset-and-recount of a retried read)."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from thermite_amd import capi, refdata

from gpu_common import (MARKER_LIMIT, MICRO_OPTS, World, assert_hits_equal, check_align, count_yclips, exonic_yclip_counts,
                        expected_batch, initial_band, micro_exon_reads, micro_exon_reference, mutate, ordinary_reads)

pytestmark = pytest.mark.gpu

_worlds = {}


def _world(key, make, wide):
    if (key, wide) not in _worlds:
        _worlds[(key, wide)] = World(make(), wide)
    return _worlds[(key, wide)]


@pytest.fixture(params=[False, True], ids=["c32", "c64"])
def micro(request):
    w = _world("micro", micro_exon_reference, request.param)
    assert int(w.t["txs"]["n_exons"].max()) > MARKER_LIMIT + 1  # the retry is armed
    return w


@pytest.fixture(params=[False, True], ids=["c32", "c64"])
def plain(request):
    return _world("plain", lambda: micro_exon_reference(with_micro=False), request.param)


N_PLANT = 320


@pytest.fixture(params=[False, True], ids=["c32", "c64"])
def planted(request):
    return _world("planted", lambda: micro_exon_reference(n_plant=N_PLANT), request.param)


def _assert_both_sides(r, n_over=50, n_under=50, n_edge=5):
    y = exonic_yclip_counts(r)
    assert (y == MARKER_LIMIT).sum() >= n_edge and (y == MARKER_LIMIT + 1).sum() >= n_edge, np.bincount(y)[60:70]
    assert (y > MARKER_LIMIT).sum() >= n_over and ((y >= 1) & (y <= MARKER_LIMIT)).sum() >= n_under
    return y


@pytest.mark.parametrize("mutated", [False, True], ids=["exact", "mutated"])
def test_boundary_and_beyond(micro, mutated):
    """91, 150, 200 and 250-base reads along the micro-exon transcripts: 64, 65 and up to 201 introns crossed"""
    bases, off, _ = micro_exon_reads(micro.t, mutated=mutated)
    for opts in (MICRO_OPTS, dict(MICRO_OPTS, intron_mode=False, multimap_score_range=3)):
        r = micro.oix.align_batch(bases, off, opts, n_threads=8)
        _assert_both_sides(r)
        check_align(micro, bases, off, opts, ref=r)


def test_armed_but_idle(micro, plain):
    """the any-width launch is enqueued over an empty list: reads of the ordinary genes and the contig only"""
    bases, off = ordinary_reads(micro.t, 3000, stream=3)
    for opts in (MICRO_OPTS, capi.CI_OPTS):
        r = micro.oix.align_batch(bases, off, opts, n_threads=8)
        y = exonic_yclip_counts(r)
        assert len(y) >= 1000 and (y >= 1).sum() >= 100 and y.max() <= MARKER_LIMIT  # spliced alignments, none retried
        check_align(micro, bases, off, opts, ref=r)
        # the same reads where nothing is armed
        assert int(plain.t["txs"]["n_exons"].max()) <= MARKER_LIMIT + 1
        check_align(plain, bases, off, opts)


def test_mixed_lists_slow_reads_then_retries(micro):
    """one batch: ordinary 91-base reads, micro-exon reads (retries) and reads beyond the fast class (the slow list):
    the any-width launch walks the slow-class reads and, behind them, whatever the other launches appended"""
    rng = np.random.default_rng(9)
    ob, oo = ordinary_reads(micro.t, 400, stream=5)
    reads = [ob[oo[i]: oo[i + 1]] for i in range(400)]
    mb, mo, planned = micro_exon_reads(micro.t, lengths=(91,), mutated=True, stride=5)
    pick = np.concatenate([rng.permutation(np.nonzero(planned > MARKER_LIMIT)[0])[:32], rng.permutation(np.nonzero(planned <= MARKER_LIMIT)[0])[:16]])
    micro_reads = [mb[mo[i]: mo[i + 1]] for i in pick]
    fwd = micro.t["text"][: int(micro.t["refs"][0]["len"])]
    lo, hi = micro.t["_gene_region"]
    long_reads = []
    for j, L in enumerate([300, 333, 450, 512, 640, 777, 1000, 1000]):
        s = int(rng.integers(lo, hi - L))
        g = mutate(rng, fwd[s: s + L], sub=0.02, indel=0.004)
        long_reads.append(refdata.revcomp(g) if j & 1 else g)
    for m in micro.t["_micro"]:  # and along a whole micro-exon transcript: more markers than the limit, in the slow class itself
        tx = micro.t["txs"][m["tx_idx"]]
        if int(tx["seq_len"]) >= 300:
            seq = micro.t["tx_seq"][int(tx["seq_off"]): int(tx["seq_off"]) + int(tx["seq_len"])]
            long_reads.append(mutate(rng, seq[:300 + 10 * len(long_reads)], sub=0.01, indel=0.003))
    for r in micro_reads + long_reads:
        reads.insert(int(rng.integers(0, len(reads) + 1)), r)
    bases, off = refdata.pack_reads(reads)
    lens = np.diff(off.astype(np.int64))
    r = micro.oix.align_batch(bases, off, MICRO_OPTS, n_threads=8)
    n_alns = np.diff(r.offsets.astype(np.int64))
    over = np.zeros(len(lens), bool)
    for i in np.nonzero(r.alns["aln_type"] == 0)[0]:
        if count_yclips(r, i) > MARKER_LIMIT:
            over[int(np.searchsorted(r.offsets, i, side="right") - 1)] = True
    fast = lens <= 255  # (the fast class ends at 255 bases at the latest)
    assert (over & (lens <= 100)).sum() >= 10          # retries out of the fast class
    assert (over & (lens >= 300)).sum() >= 1           # beyond the limit inside the slow class
    assert ((lens >= 300) & (n_alns > 0)).sum() >= 8   # slow-class reads that align
    assert (fast & ~over & (n_alns > 0)).sum() >= 300
    check_align(micro, bases, off, MICRO_OPTS, ref=r)


def test_team_kernel_meets_the_retry(planted):
    """A read that starts in the planted first exon has more than TEAM_HITS = 256 seed hits (the workgroup-per-read kernel
    takes it) and its best alignment, along the transcript, crosses more than 64 introns: the team's lead wave appends the
    read to the retry list.  91-base reads at 0.66: band +-31."""
    w = planted
    m = w.t["_micro"][0]
    assert m["strand"] and all(b - a == 1 for a, b in m["exons"][1:-1])
    tx = w.t["txs"][m["tx_idx"]]
    seq = w.t["tx_seq"][int(tx["seq_off"]): int(tx["seq_off"]) + int(tx["seq_len"])]
    rng = np.random.default_rng(4)
    reads = []
    for o in range(35, 47):  # 60 - o bases of the exon (the seed: 25..14 bases), 31 + o one-base exons behind it
        rd = seq[o: o + 91]
        reads.append(rd)
        p = int(rng.integers(60 - o + 2, 89))
        e = list(rd)
        e[p] = ord("A") if e[p] != ord("A") else ord("C")
        reads.append(np.array(e, np.uint8))
    ob, oo = ordinary_reads(w.t, 600, stream=8)
    reads += [ob[oo[i]: oo[i + 1]] for i in range(600)]
    order = rng.permutation(len(reads))
    team_reads = np.argsort(order)[:24]  # where the 24 reads above went
    bases, off = refdata.pack_reads([reads[i] for i in order])
    opts = dict(MICRO_OPTS, min_seed_len=14)
    assert initial_band(opts, 91) <= 63
    a = w.aligner(opts)
    mo, _ = a.smems_batch(bases, off, opts["min_seed_len"])
    a.close()
    hits = np.diff(mo.astype(np.int64))
    assert (hits[team_reads] >= 256).all() and (hits[team_reads] <= 60000).all(), hits[team_reads]
    r = w.oix.align_batch(bases, off, opts, n_threads=8)
    for i in team_reads:
        a0, a1 = int(r.offsets[i]), int(r.offsets[i + 1])
        assert a1 > a0 and r.alns[a0]["aln_type"] == 0 and count_yclips(r, a0) > MARKER_LIMIT, i
    check_align(w, bases, off, opts, ref=r)


def test_pool_overflow_on_retried_reads(micro):
    """the op pool or the candidate pool overflows in a batch with retried reads: grow, replay, same result and counters"""
    bases, off, _ = micro_exon_reads(micro.t, mutated=True)
    ob, oo = ordinary_reads(micro.t, 500, stream=6)
    n = len(off) - 1
    b2 = np.concatenate([bases, ob])
    o2 = np.concatenate([off, oo[1:] + off[-1]]).astype("<u8")
    r = micro.oix.align_batch(b2, o2, MICRO_OPTS, n_threads=8)
    _assert_both_sides(r)
    assert n > 500
    for caps in (dict(ops_cap=8192), dict(cand_cap=64), dict(cand_cap=32, ops_cap=4096)):
        check_align(micro, b2, o2, MICRO_OPTS, pool_caps=caps, ref=r)


def orc_ops(ops, a):
    return orc.decode_ops(ops[int(a["ops_off"]): int(a["ops_off"]) + int(a["ops_len"])])


def _hits(w, bases, off, opts, rng, narrow):
    hit_off, hits = w.a.smems_batch(bases, off, opts["min_seed_len"])
    lens = np.diff(off.astype(np.int64))
    per_hit_len = np.repeat(lens, np.diff(hit_off.astype(np.int64)))
    bw0 = np.array([initial_band(opts, int(L)) for L in per_hit_len], "<u4")
    if narrow:
        bw = (bw0 * (0.3 + 0.7 * rng.random(len(bw0)))).astype("<u4")
        xd = (bw + rng.integers(0, 6, len(bw))).astype("<i4")
    else:
        bw, xd = bw0, bw0.astype("<i4")
    return hit_off, hits, bw, xd, int(bw0.max(initial=0))


@pytest.mark.parametrize("mutated", [False, True], ids=["exact", "mutated"])
def test_per_hit_entry_point(micro, mutated):
    """thm_align_seed_hits_batch on the hits of the micro-exon reads (initial and narrowed bands): records with more than 64
    markers come from the entry point's own retry launch"""
    rng = np.random.default_rng(12)
    bases, off, _ = micro_exon_reads(micro.t, mutated=mutated, stride=7 if not mutated else 21)
    for narrow in (False, True):
        hit_off, hits, bw, xd, max_bw = _hits(micro, bases, off, MICRO_OPTS, rng, narrow)
        exp = expected_batch(micro, bases, off, hit_off, hits, bw, xd, max_bw)
        e_alns, e_ops, e_st = exp
        assert not e_st.any()
        y = np.array([sum(1 for o in orc_ops(e_ops, a) if isinstance(o, tuple) and o[0] == "Yclip") for a in e_alns])
        assert (y > MARKER_LIMIT).sum() >= 50 and ((y >= 1) & (y <= MARKER_LIMIT)).sum() >= 50, (narrow, np.bincount(y))
        got = micro.a.align_seed_hits(bases, off, hit_off, hits, bw, xd, max_bw)
        assert not got[2].any()
        assert_hits_equal(got, exp, "narrow" if narrow else "initial")


def test_per_hit_entry_point_armed_but_idle(micro):
    """hits of ordinary reads only, on the index that arms the retry: its launch runs over an empty list"""
    rng = np.random.default_rng(13)
    bases, off = ordinary_reads(micro.t, 250, stream=14, sub_rate=0.03, indel_rate=0.006)
    hit_off, hits, bw, xd, max_bw = _hits(micro, bases, off, capi.CI_OPTS, rng, False)
    assert len(hits) >= 200
    exp = expected_batch(micro, bases, off, hit_off, hits, bw, xd, max_bw)
    y = np.array([sum(1 for o in orc_ops(exp[1], a) if isinstance(o, tuple) and o[0] == "Yclip") for a in exp[0]])
    assert not exp[2].any() and y.max() <= MARKER_LIMIT and (y >= 1).sum() >= 20
    got = micro.a.align_seed_hits(bases, off, hit_off, hits, bw, xd, max_bw)
    assert_hits_equal(got, exp, "idle")
