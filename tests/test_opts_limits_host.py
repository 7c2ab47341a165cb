"""CPU: the inputs of tests/test_gpu_opts_limits.py, pinned with the oracle alone.  The GPU tests compare the device
with the oracle at the limits of thm_align_opts; they mean something only if the read sets reach the conditions the
limits are about -- multimappers that need a band after the first accepted alignment, reads that an exact band of 0
aligns and reads it does not, seed lengths that leave hits and seed lengths that leave none.  That is asserted here,
where no device is involved."""
import numpy as np
import pytest

from oracle import pyoracle as orc

import opts_limits_common as ol


@pytest.fixture(scope="module")
def rep():
    t, pos = ol.rep_tables()
    bases, off = ol.rep_reads(t, pos)
    return orc.Index(t), bases, off


@pytest.fixture(scope="module")
def syn():
    t = ol.syn_tables()
    bases, off = ol.syn_reads(t)
    return orc.Index(t), bases, off


@pytest.fixture(scope="module")
def rep_by_range(rep):
    oix, bases, off = rep
    return {v: oix.align_batch(bases, off, ol.rep_opts(v), n_threads=8) for v, _ in ol.RANGES}


def n_alns(r):
    return np.diff(r.offsets.astype(np.int64))


def test_rep_read_set(rep):
    oix, bases, off = rep
    assert len(off) == 241 and (np.diff(off.astype(np.int64)) == ol.L).all()
    r = oix.align_batch(bases, off, ol.REP_OPTS, n_threads=8)
    assert r.counters[15] == 0
    assert 240 <= len(r.alns) <= 1000    # range 1: about two alignments a read


def test_ranges_are_defined_in_the_reference(rep_by_range):
    for v, name in ol.RANGES:
        assert rep_by_range[v].counters[15] == 0, name
        # neither sum of align_read overflows: read.len() + range in usize, max_aln_score - (range as i32) in i32
        assert 65535 + v < 2 ** 64
        as_i32 = (v & 0xFFFFFFFF) - (2 ** 32 if v & 0x80000000 else 0)
        assert -2 ** 31 <= 65535 - as_i32 <= ol.I32_MAX, name


def test_wide_range_needs_the_band(rep_by_range):
    """Under a range of 2^31 - 1 every alignment above the threshold stays, and the band never narrows.  A band of 0 after
    the first accepted alignment -- what `L + range - score` gives once it has wrapped -- cannot give a later alignment
    with a gap: at least 100 reads have three or more alignments of which at least two hold an Ins or a Del."""
    r = rep_by_range[ol.I32_MAX]
    n = n_alns(r)
    assert len(r.alns) >= 2000 and n.max() >= 20
    need_band = sum(1 for i in range(len(n)) if n[i] >= 3 and ol.n_gapped(r, i) >= 2)
    print("reads with >= 3 alignments, >= 2 of them gapped: %d; alignments %d, at most %d a read" % (need_band, len(r.alns), n.max()))
    assert need_band >= 100


def test_ranges_that_never_narrow_agree(rep_by_range):
    """a range of 65535 or more never narrows band or X-drop; where its i32 value also keeps every alignment the results
    are the same"""
    r1000 = rep_by_range[1000]
    for v in (ol.I32_MAX - 91, ol.I32_MAX - 90, ol.I32_MAX):
        assert ol.results_equal(rep_by_range[v], r1000), v


def test_truncated_ranges(rep_by_range):
    """2^32 - 1 is -1 as i32: the final retain asks for score >= max + 1 and no read keeps an alignment.  2^32 + k is k as
    i32 for the comparisons, but the band does not narrow as it does for a range of k."""
    r = rep_by_range[2 ** 32 - 1]
    assert len(r.alns) == 0 and r.counters[1] == 0
    for v in (2 ** 32, 2 ** 32 + 1, 2 ** 32 + 6, 2 ** 63):
        assert len(rep_by_range[v].alns) >= 240, v


def test_low_bits_alone_give_another_result(rep):
    """the device's supposed fault for ranges of 2^32 and more -- narrowing by the low 32 bits -- would show: the oracle's
    result for 2^32 + k differs from its result for k in records or in DP work"""
    oix, bases, off = rep
    differ = 0
    for k in (0, 1, 6):
        lo = oix.align_batch(bases, off, ol.rep_opts(k), n_threads=8)
        hi = oix.align_batch(bases, off, ol.rep_opts(2 ** 32 + k), n_threads=8)
        differ += (not ol.results_equal(lo, hi)) or lo.counters[10] != hi.counters[10]
    assert differ == 3


@pytest.fixture(scope="module")
def syn_by_case(syn):
    oix, bases, off = syn
    out = {}
    for name, (opts, which) in ol.SCORE_CASES.items():
        b, o = ol.syn_case_reads(bases, off, which)
        out[name] = (b, o, oix.align_batch(b, o, opts, n_threads=8))
    return out


def test_score_thresholds(syn_by_case):
    for name, (_, _, r) in syn_by_case.items():
        assert r.counters[15] == 0, name
    n = n_alns(syn_by_case["pct1"][2])
    print("percentage 1.0: %d of %d reads aligned" % ((n > 0).sum(), len(n)))
    assert (n > 0).sum() >= 500 and (n == 0).sum() >= 300
    b, o, r = syn_by_case["pct1_cut"]
    lens = np.diff(o.astype(np.int64))
    assert lens.min() == 0 and lens.max() == ol.L and len(np.unique(lens)) > 60
    assert (n_alns(r) > 0).sum() >= 100
    for name in ("min200", "min_i32max"):
        r = syn_by_case[name][2]
        assert len(r.alns) == 0 and r.counters[8] >= 1500 and r.counters[9] > 0, name   # hits extended, none accepted
    for name in ("pct0_min-7", "pct0_min_i32min"):
        r = syn_by_case[name][2]
        assert (n_alns(r) > 0).sum() == ol.N_SEED, name
    assert ol.results_equal(syn_by_case["pct0_min-7"][2], syn_by_case["pct0_min_i32min"][2])
    assert ol.band_at_L(ol.SCORE_CASES["pct0_min-7"][0]) == ol.L and ol.band_at_L(ol.SCORE_CASES["pct1"][0]) == 0


def test_seed_lengths(syn):
    oix, bases, off = syn
    b, o = ol.first_reads(bases, off, ol.N_SEED)
    for k in ol.SEED_LENS:
        m = oix.all_smems(b, o, k)
        r = oix.align_batch(b, o, ol.seed_opts(k), n_threads=8)
        assert r.counters[15] == 0, k
        if k < ol.L:
            assert len(m.mems) >= 300 and r.counters[8] >= 1000 and (n_alns(r) > 0).sum() >= 250, k
        elif k == ol.L:   # only a read that matches as a whole has a seed, and its alignment is that match
            assert len(m.mems) >= 50 and (m.mems["len"] == ol.L).all() and (m.mems["query_idx"] == 0).all()
            assert r.counters[8] == len(m.mems) and len(r.alns) > 0 and (r.alns["score"] == ol.L).all()
        else:
            assert len(m.mems) == 0 and r.counters[7] == 0 and r.counters[8] == 0 and len(r.alns) == 0, k


def test_sequence_steps_differ(rep):
    """the steps of the set_opts sequence give different results on their read set, so that a run under the options of
    the step before -- or of the step after, in the replay case -- is seen"""
    sets = {"rep": rep, "sim": (rep[0],) + tuple(ol.sim_reads(ol.rep_tables()[0]))}
    res = []
    for name, opts, which in ol.SEQUENCE:
        oix, b, o = sets[which]
        r = oix.align_batch(b, o, opts, n_threads=8)
        assert r.counters[15] == 0, name
        res.append(r)
    for i in range(1, len(ol.SEQUENCE)):
        name, opts, which = ol.SEQUENCE[i]
        oix, b, o = sets[which]
        before = oix.align_batch(b, o, ol.SEQUENCE[i - 1][1], n_threads=8)
        assert (not ol.results_equal(before, res[i])) or not np.array_equal(before.counters, res[i].counters), name
    # the replay case: started under BASE, fetched after set_opts(PCT03), on the sim reads (the rep reads' records are the
    # same under both: only their DP work differs)
    oix, b, o = sets["sim"]
    x, y = oix.align_batch(b, o, ol.BASE, n_threads=8), oix.align_batch(b, o, ol.PCT03, n_threads=8)
    print("sim reads: %d alignments under BASE, %d under PCT03" % (len(x.alns), len(y.alns)))
    assert len(y.alns) >= len(x.alns) + 10 and (np.diff(x.offsets.astype(np.int64)) > 0).sum() >= 400
    assert [ol.band_at_L(s[1]) for s in ol.SEQUENCE[:5]] == [31, 61, 91, 31, 0]
