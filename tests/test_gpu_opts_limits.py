"""-m gpu: read-level parity with the oracle at the limits of thm_align_opts, and thm_aligner_set_opts between the runs of
one aligner, at both coordinate widths.  The read sets and the case table are in opts_limits_common.py; that they reach
the conditions the cases are about is asserted without a device in test_opts_limits_host.py.

Every comparison is byte equality through gpu_common.check_align (both extend paths, records, op bytes, counters) or,
where one aligner lives through several runs, assert_batch_equal and the oracle's running counter sums.

  A  multimap_score_range up to 2^63: the band narrows by min(band, L + range - score) with the untruncated range
     (reference src/aligner.rs:162-171), only the comparisons take `range as i32` (:156, :178)
  B  score thresholds: a percentage of 1.0 (band 0), min_aln_score above L and at both ends of i32
  C  min_seed_len 1, 2, L, L + 1, 65535; 0 and 65536 are refused by every entry point that takes one
  D  the struct as C sees it: intron_mode other than 0 / 1, reserved, percentages outside [0, 1] and -0.0
  E  set_opts between runs, between upload and run, refused, and between run and fetch of a run that has to replay"""
import ctypes as C

import numpy as np
import pytest

from thermite_amd import capi

import opts_limits_common as ol
from gpu_common import World, assert_batch_equal, assert_counters_match, check_align, check_smems

pytestmark = pytest.mark.gpu

WIDTHS = pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def reads(which):
    """(tables, bases, offsets) of "rep", "sim" (rep's world too), "syn" (1500 reads) or "syn_seed" (the first 300)"""
    def make():
        if which == "rep":
            t, pos = ol.rep_tables()
            return (t,) + tuple(ol.rep_reads(t, pos))
        if which == "sim":
            t = reads("rep")[0]
            return (t,) + tuple(ol.sim_reads(t))
        if which == "syn":
            t = ol.syn_tables()
            return (t,) + tuple(ol.syn_reads(t))
        t, b, o = reads("syn")
        return (t,) + tuple(ol.first_reads(b, o, ol.N_SEED))
    return _once(("reads", which), make)


def world(which, wide):
    name = "syn" if which.startswith("syn") else "rep"
    return _once(("world", name, wide), lambda: World(reads(name)[0], wide))


def oracle(which, opts, bases=None, off=None, key=None):
    """the oracle's result for a read set under `opts`, computed once (both widths share it)"""
    def make():
        t, b, o = reads(which)
        if bases is not None:
            b, o = bases, off
        r = world(which, False).oix.align_batch(b, o, opts, n_threads=8)
        assert r.counters[15] == 0, "oracle saw reads where the reference would panic"
        return r
    return _once(("oracle", which, key, tuple(sorted(opts.items()))), make)


def raw_opts(o, intron_mode=None, reserved=0):
    """thm_align_opts as a C caller fills it (capi.Aligner._mk coerces intron_mode to 0 / 1 and zeroes reserved)"""
    return capi.Opts(o["min_seed_len"], o["min_aln_score_percent"], o["min_aln_score"], o["multimap_score_range"],
                     int(bool(o["intron_mode"])) if intron_mode is None else intron_mode, reserved)


def set_raw(a, o):
    return capi.lib().thm_aligner_set_opts(a.h, C.byref(o))


# ------------------------------------------------------------------ A: multimap_score_range
@WIDTHS
@pytest.mark.parametrize("value", [v for v, _ in ol.RANGES], ids=ol.RANGE_IDS)
def test_multimap_score_range(value, wide):
    _, bases, off = reads("rep")
    opts = ol.rep_opts(value)
    ref = oracle("rep", opts)
    g = check_align(world("rep", wide), bases, off, opts, ref=ref)
    if value == 2 ** 32 - 1:
        assert len(g.alns) == 0 and g.n_failed == 0


@WIDTHS
def test_out_of_contract_ranges_are_refused(wide):
    """The reference itself overflows on them: read.len() + range in usize for a range above 2^64 - 1 - 65535, and
    max_aln_score - (range as i32) in i32 where that cast is negative and max(65535, min_aln_score) minus it exceeds
    i32::MAX.  thm_aligner_set_opts answers THM_ERR_OUT_OF_CONTRACT and the options in force stay."""
    _, bases, off = reads("rep")
    w = world("rep", wide)
    ref = oracle("rep", ol.REP_OPTS)
    a = w.aligner(ol.REP_OPTS)
    for o in (ol.rep_opts(2 ** 31), ol.rep_opts(2 ** 31 + 65535), ol.rep_opts(2 ** 64 - 65535), ol.rep_opts(2 ** 64 - 1),
              dict(ol.rep_opts(2 ** 32 - 1), min_aln_score=ol.I32_MAX)):
        assert set_raw(a, raw_opts(o)) == capi.ERR_OUT_OF_CONTRACT, o
        with pytest.raises(capi.ThermiteError) as e:
            capi.Aligner(w.ix, o)
        assert e.value.code == capi.ERR_OUT_OF_CONTRACT
    assert_batch_equal(a.align_batch(bases, off), ref)
    # the other side of each rule
    for o in (ol.rep_opts(2 ** 32 - 1), ol.rep_opts(2 ** 31 + 65536), ol.rep_opts(2 ** 64 - 1 - 65535),
              dict(ol.rep_opts(2 ** 32 - 1), min_aln_score=ol.I32_MAX - 1)):
        assert set_raw(a, raw_opts(o)) == capi.OK, o
    a.close()


# ------------------------------------------------------------------ B: score thresholds
@WIDTHS
@pytest.mark.parametrize("name", list(ol.SCORE_CASES))
def test_score_thresholds(name, wide):
    opts, which = ol.SCORE_CASES[name]
    _, bases, off = reads("syn")
    b, o = ol.syn_case_reads(bases, off, which)
    ref = oracle("syn", opts, b, o, key=which)
    g = check_align(world("syn", wide), b, o, opts, ref=ref)
    if name.startswith("min"):
        assert len(g.alns) == 0


# ------------------------------------------------------------------ C: seed length
@WIDTHS
@pytest.mark.parametrize("k", ol.SEED_LENS)
def test_seed_lengths(k, wide):
    _, b, o = reads("syn_seed")
    w = world("syn", wide)
    check_smems(w, b, o, k)
    opts = ol.seed_opts(k)
    g = check_align(w, b, o, opts, ref=oracle("syn_seed", opts))
    if k > ol.L:
        assert len(g.alns) == 0


@WIDTHS
@pytest.mark.parametrize("k", ol.SEED_LENS_REFUSED)
def test_seed_lengths_refused(k, wide):
    """thm_aligner_create, thm_aligner_set_opts and thm_smems_batch answer THM_ERR_INVALID_ARG; the aligner goes on under
    the options it had"""
    _, b, o = reads("syn_seed")
    w = world("syn", wide)
    ref = oracle("syn_seed", ol.SYN_OPTS)
    with pytest.raises(capi.ThermiteError) as e:
        capi.Aligner(w.ix, ol.seed_opts(k))
    assert e.value.code == capi.ERR_INVALID_ARG
    a = w.aligner(ol.SYN_OPTS)
    assert_batch_equal(a.align_batch(b, o), ref)
    with pytest.raises(capi.ThermiteError) as e:
        a.set_opts(ol.seed_opts(k))
    assert e.value.code == capi.ERR_INVALID_ARG
    assert_batch_equal(a.align_batch(b, o), ref)
    with pytest.raises(capi.ThermiteError) as e:
        a.smems_batch(b, o, k)
    assert e.value.code == capi.ERR_INVALID_ARG
    a.reset_counters()
    g = a.align_batch(b, o)
    assert g.n_failed == 0
    assert_batch_equal(g, ref)
    assert_counters_match(a.counters(), ref.counters, "after the refused calls")
    a.close()


# ------------------------------------------------------------------ D: the struct as C sees it
@WIDTHS
def test_struct_as_c_sees_it(wide):
    _, b, o = reads("syn_seed")
    w = world("syn", wide)
    on = oracle("syn_seed", ol.SYN_OPTS)
    off_opts = dict(ol.SYN_OPTS, intron_mode=False)
    off = oracle("syn_seed", off_opts)
    assert len(off.alns) < len(on.alns)
    a = w.aligner(off_opts)

    def run_is(ref, what):
        for tpr in (False, True):
            a.debug_set_flags(tpr=tpr)
            a.reset_counters()
            g = a.align_batch(b, o)
            assert g.n_failed == 0 and g.status is None, what
            assert_batch_equal(g, ref)
            assert_counters_match(a.counters(), ref.counters, (what, tpr))

    run_is(off, "intron_mode 0")
    for v in (2, -1, -2 ** 31, 256):   # any nonzero value is `true`
        assert set_raw(a, raw_opts(off_opts)) == capi.OK
        assert set_raw(a, raw_opts(ol.SYN_OPTS, intron_mode=v)) == capi.OK
        run_is(on, "intron_mode %d" % v)
    for rsv in (1, -1):
        assert set_raw(a, raw_opts(off_opts, reserved=rsv)) == capi.OK
        run_is(off, "reserved %d" % rsv)
    # percentages outside [0, 1] are refused (src/main.rs:46-49) and the options in force stay
    for pct in (float("nan"), -1e-9, 1.0000001, float("inf"), -float("inf")):
        assert set_raw(a, raw_opts(dict(ol.SYN_OPTS, min_aln_score_percent=pct))) == capi.ERR_INVALID_ARG, pct
        with pytest.raises(capi.ThermiteError) as e:
            capi.Aligner(w.ix, dict(ol.SYN_OPTS, min_aln_score_percent=pct))
        assert e.value.code == capi.ERR_INVALID_ARG
    run_is(off, "after the refused percentages")
    # -0.0 is 0.0
    zero = dict(ol.SYN_OPTS, min_aln_score_percent=0.0)
    assert set_raw(a, raw_opts(dict(zero, min_aln_score_percent=-0.0))) == capi.OK
    run_is(oracle("syn_seed", zero), "-0.0")
    a.close()


# ------------------------------------------------------------------ E: set_opts between runs
@WIDTHS
def test_set_opts_between_runs(wide):
    """One aligner, ol.SEQUENCE: after every step the records and op bytes are the oracle's for the options in force and
    the counters its running sums.  The read set is uploaded again only where it changes, and set_opts comes between the
    upload and the run; the problem-parallel path is on in every second step.  Inside the sequence: a refused set_opts,
    and a set_opts between thm_batch_run and the fetch of a run that overflows its pools -- the replay is the run's own,
    under the options it was started with."""
    w = world("rep", wide)
    a = w.aligner(ol.SEQUENCE[0][1])
    a.reset_counters()
    total = np.zeros(capi.N_COUNTERS, "<u8")
    uploaded = [None]

    def upload(which, force=False):
        if force or uploaded[0] != which:
            _, b, o = reads(which)
            a.upload(b, o)
            uploaded[0] = which

    def fetched_is(opts, which, what):
        ref = oracle(which, opts)
        g = a.fetch()
        assert g.n_failed == 0 and g.status is None, what
        assert_batch_equal(g, ref)
        total[:] += ref.counters
        assert_counters_match(a.counters(), total, what)

    for i, (name, opts, which) in enumerate(ol.SEQUENCE):
        a.debug_set_flags(tpr=bool(i & 1))
        upload(which)
        if i > 0:
            a.set_opts(opts)
        a.run()
        fetched_is(opts, which, name)
        if name == "pct03":
            with pytest.raises(capi.ThermiteError) as e:
                a.set_opts(dict(opts, min_aln_score_percent=1.5))
            assert e.value.code == capi.ERR_INVALID_ARG
            a.run()
            fetched_is(opts, which, "after the refused set_opts")
            # the run starts under BASE with pools that must overflow; the options change before the fetch replays it
            for tpr in (False, True):
                a.debug_set_flags(tpr=tpr)
                a.set_opts(ol.BASE)
                upload("sim", force=True)
                replays = a.debug_set_pool_caps(**ol.REPLAY_CAPS)
                a.run()
                a.set_opts(ol.PCT03)
                fetched_is(ol.BASE, "sim", ("replay after set_opts", tpr))
                assert a.debug_set_pool_caps() > replays, "the small pools did not overflow"
                # the new options hold from the next run on
                a.run()
                fetched_is(ol.PCT03, "sim", ("run after the replay", tpr))
    a.close()


