"""-m gpu: the per-base coverage tracks of a run, built on the device (kernels_coverage.hip, thm_coverage).  Every case
compares what a fetch returns -- runs, the view's sums, totals, windows of depths -- with the expectation of
tests/cov_common.py, which is written from the contract in include/thermite_io.h and deposits the oracle's alignments (or
a view made by hand) into per-base arrays."""
import contextlib
import os
import re

import numpy as np
import pytest

import bam_common as bc
import cigar_common as cc
import cov_common as cv
import quant_common as qc
from gpu_common import World
from thermite_amd import capi

pytestmark = pytest.mark.gpu

_memo = {}
KNOBS = ("THM_COVERAGE", "THM_QUANT", "THM_BAM_SORT", "THM_BAM_INDEX", "THM_BAM_DEVICE", "THM_FASTQ_DEVICE")
TILE = capi.COV_TILE


def _world(key, wide=False):
    if (key, wide) not in _memo:
        t = {"test_ref": lambda: bc.tables("test_ref"), "syn": qc.syn_tables, "shape": cv.shape_tables}[key]()
        _memo[(key, wide)] = World(t, wide)
    return _memo[(key, wide)]


def _syn_run():
    """(bases, offsets, the oracle's result) of the synthetic run; the oracle runs once"""
    if "run" not in _memo:
        w = _world("syn")
        bases, off = qc.syn_reads(w.t)
        r = w.oix.align_batch(bases, off, capi.CI_OPTS, n_threads=8)
        assert r.counters[15] == 0
        _memo["run"] = (bases, off, r)
    return _memo["run"]


def _syn_expect(flags):
    if ("exp", flags) not in _memo:
        _memo[("exp", flags)] = cv.from_oracle(_world("syn").t, flags, _syn_run()[2])
    return _memo[("exp", flags)]


def _part(bases, off, lo, hi):
    b0 = int(off[lo])
    return bases[b0: int(off[hi])], (off[lo: hi + 1] - off[lo]).astype("<u8")


def _add_reads(a, c, bases, off):
    a.upload(bases, off)
    a.run()
    return c.add()


def _raises(f):
    with pytest.raises(capi.ThermiteError) as e:
        f()
    return e.value


def _batch_totals(info):
    return {k: info[k] for k in cv.TOTAL_NAMES + ["track"]}


def _check_all(c, exp, what=""):
    """every track over all contigs, and contig by contig"""
    n_sq = len(exp.lens)
    for k in range(cv.n_tracks(exp.flags)):
        cv.check_result(c.fetch(k, 0, n_sq), exp, k, 0, n_sq, what)
        for s in range(n_sq):
            cv.check_result(c.fetch(k, s, 1), exp, k, s, 1, "%s contig %d" % (what, s))


def _pack(c, flags, n_sq):
    return b"".join(c.fetch(k, 0, n_sq).runs.tobytes() for k in range(cv.n_tracks(flags)))


# ------------------------------------------------------------------ 1. config 1 through the aligner
@pytest.mark.parametrize("flags", cv.ALL_FLAGS)
def test_config_1_gives_the_hand_tables(flags):
    w = _world("test_ref")
    rs = bc.read_set("test_query", w.t)
    b = bc.batch_of(rs)
    a = w.aligner(rs["opts"])
    c = capi.Coverage(a, flags)
    info = _add_reads(a, c, b["bases"], b["offsets"])
    res = [c.fetch(k, 0, 4) for k in range(cv.n_tracks(flags))]
    cv.assert_golden(w.t, flags, lambda k: res[k].runs, res[0].totals)
    assert _batch_totals(info) == res[0].totals and info["held_bytes"] > 0
    # the run of another_seq ends on the contig's last base
    if flags == 0:
        assert cv.table(c.fetch(0, 1, 1).runs, 1) == [(8, 12, 1)] and c.depth(0, 1, 0, 12).tolist() == [0] * 8 + [1] * 4
    c.close()
    a.close()


def test_create_refuses_what_it_must():
    w = _world("test_ref")
    rs = bc.read_set("test_query", w.t)
    # the names precondition of the BAM layer, with its message
    t = {k: v for k, v in w.t.items() if k not in ("names", "tx_ids", "gene_ids", "gene_names")}
    ix = capi.Index(t)
    a = capi.Aligner(ix, rs["opts"])
    a.upload_reads(bc.batch_of(rs))
    a.run()
    e_bam = _raises(a.fetch_bam)
    e = _raises(lambda: capi.Coverage(a))
    assert (e.code, str(e)) == (e_bam.code, str(e_bam)) and e.code == capi.ERR_INVALID_ARG and "names" in str(e)
    a.close()
    ix.close()
    # unknown flag bits
    a = w.aligner(rs["opts"])
    assert _raises(lambda: capi.Coverage(a, 4)).code == capi.ERR_INVALID_ARG
    # a cap one below the need: the message holds both numbers; the need itself is enough
    e = _raises(lambda: capi.Coverage(a, 3, 1))
    assert e.code == capi.ERR_OOM
    need = int(re.search(r"need (\d+) bytes, the cap is 1\b", str(e)).group(1))
    assert need >= 4 * 4 * sum(cv.sq_lengths(w.t))
    e = _raises(lambda: capi.Coverage(a, 3, need - 1))
    assert e.code == capi.ERR_OOM and str(need) in str(e) and str(need - 1) in str(e)
    c = capi.Coverage(a, 3, need)
    # a fetch and a depth call check their arguments
    for f in (lambda: c.fetch(4, 0, 1), lambda: c.fetch(0, 3, 2), lambda: c.fetch(0, 5, 0), lambda: c.depth(0, 4, 0, 1), lambda: c.depth(4, 0, 0, 1),
              lambda: c.depth(0, 1, 0, 13), lambda: c.depth(0, 1, 12, 1), lambda: c.depth(0, 0, 0, (1 << 24) + 1)):
        assert _raises(f).code == capi.ERR_INVALID_ARG
    assert len(c.fetch(0, 4, 0).runs) == 0 and len(c.depth(0, 1, 12, 0)) == 0
    c.close()
    a.close()


# ------------------------------------------------------------------ 2. the synthetic run
@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
def test_synthetic_run_against_the_expectation(wide):
    bases, off, r = _syn_run()
    w = _world("syn", wide)
    a = w.aligner(capi.CI_OPTS)
    n = cv.sq_lengths(w.t)[0]
    for flags in cv.ALL_FLAGS:
        exp = _syn_expect(flags)
        c = capi.Coverage(a, flags)
        info = _add_reads(a, c, bases, off) if flags == 0 else c.add()
        assert _batch_totals(info) == exp.totals
        _check_all(c, exp, "flags %d" % flags)
        assert exp.totals["n_alns"] == len(r.alns)
        for k in range(cv.n_tracks(flags)):
            # windows that start mid-tile, end on the contig's last base, hold one base
            for start, m in ((0, 1), (TILE + 17, 3 * TILE), (n - 5000, 5000), (n - 1, 1), (TILE - 1, 2), (int(exp.runs(k)["start"][0]), 300)):
                assert np.array_equal(c.depth(k, 0, start, m), exp.depth(k, 0)[start: start + m]), (flags, k, start, m)
        c.close()
    a.close()


# ------------------------------------------------------------------ 3. batching, order, reset, twice
def test_batches_in_any_cut_and_order_give_the_same_bytes():
    bases, off, r = _syn_run()
    w = _world("syn")
    flags = cv.STRANDED | cv.MULTI
    exp = _syn_expect(flags)
    want = b"".join(exp.runs(k).tobytes() for k in range(4))
    n = len(off) - 1
    cuts = [0, 1, 64, 128, 193, n]   # batches of 1, 63, 64, 65 reads and the rest
    a = w.aligner(capi.CI_OPTS)
    c = capi.Coverage(a, flags)
    for order in (range(5), reversed(range(5))):
        for k in order:
            _add_reads(a, c, *_part(bases, off, cuts[k], cuts[k + 1]))
        assert _pack(c, flags, 1) == want
        assert c.fetch(0, 0, 1).totals == exp.totals
        # reset empties the object, which goes on
        c.reset()
        z = c.fetch(0, 0, 1)
        assert len(z.runs) == 0 and z.n_bases == 0 and z.totals == cv.Expect(w.t, flags).totals and not c.depth(3, 0, 0, 4000).any()
    # one batch added 20 times: the memory stays, every depth is 20-fold
    _add_reads(a, c, *_part(bases, off, cuts[3], cuts[4]))
    once = [c.fetch(k, 0, 1) for k in range(4)]
    c.reset()
    first = c.add()
    for _ in range(19):
        info = c.add()
        assert info["held_bytes"] == first["held_bytes"] and _batch_totals(info) == _batch_totals(first)
    assert first["n_alns"] >= 60
    for k in range(4):
        got = c.fetch(k, 0, 1)
        x = once[k].runs.copy()
        x["depth"] *= 20
        cv.assert_runs_equal(got.runs, x, "20 adds, track %d" % k)
        assert got.n_bases == 20 * once[k].n_bases == got.totals["track"][k]["n_bases"] and got.n_covered == once[k].n_covered
    c.close()
    a.close()


def test_adding_a_run_twice_doubles_every_depth():
    bases, off, r = _syn_run()
    w = _world("syn")
    a = w.aligner(capi.CI_OPTS)
    c = capi.Coverage(a, cv.MULTI)
    _add_reads(a, c, bases, off)
    c.add()
    _check_all(c, _syn_expect(cv.MULTI).scaled(2), "twice")
    c.close()
    a.close()


# ------------------------------------------------------------------ 4. the shapes of add_view
SHAPES = ["empty", "no_alignments", "whole_contig", "abutting", "tile_span", "tile_edge", "hot", "forty_introns", "one_read_5000", "both_strands", "long_run",
          "later_add"]


@pytest.mark.parametrize("name", SHAPES)
def test_add_view_shapes(name):
    w = _world("shape")
    for flags in (0, cv.STRANDED | cv.MULTI):
        c = capi.Coverage(w.a, flags)
        exp = cv.Expect(w.t, flags)
        for view in cv.shape_cases(w.t, TILE)[name]:
            info = c.add_view(*view)
            assert _batch_totals(info) == exp.add(*view), (name, flags)
            _check_all(c, exp, "%s flags %d" % (name, flags))
        for k, s, start, n in cv.shape_windows(TILE):
            if k < cv.n_tracks(flags):
                assert np.array_equal(c.depth(k, s, start, n), exp.depth(k, s)[start: start + n]), (name, flags, k, s, start, n)
        cv.assert_shape(name, flags, exp, TILE)
        cv.check_invariants(exp)
        c.close()


def test_a_bad_view_is_refused_and_the_next_fetch_is_unchanged():
    w = _world("shape")
    c = capi.Coverage(w.a, 3)
    good = cv.shape_cases(w.t, TILE)["both_strands"][0]
    c.add_view(*good)
    before = _pack(c, 3, 3), c.fetch(0, 0, 3).totals
    for name, bad in cv.bad_views(w.t).items():
        e = _raises(lambda: c.add_view(*bad))
        assert e.code == capi.ERR_INVALID_ARG and "alignment 1" in str(e), (name, str(e))
    # a digest that understates ref_len passes the host's check: the device's pass finds the walk's end
    off, alns, dig, words = cv.bad_views(w.t)["past_the_contig"]
    lie = dig.copy()
    lie["ref_len"][1] = 50
    e = _raises(lambda: c.add_view(off, alns, lie, words))
    assert e.code == capi.ERR_INVALID_ARG and "alignment 1" in str(e) and "contig" in str(e)
    assert _raises(lambda: c.add_view(off[::-1].copy(), alns, dig, words)).code == capi.ERR_INVALID_ARG
    assert (_pack(c, 3, 3), c.fetch(0, 0, 3).totals) == before
    # the alignment that ends exactly at the contig's length is taken
    fit = words.copy()
    fit[-1] -= 1 << 4
    dig2 = dig.copy()
    dig2["ref_len"][1] -= 1
    c.add_view(off, alns, dig2, fit)
    assert cv.table(c.fetch(0, 1, 1).runs, 1) == [(950, 970, 1), (980, 1000, 1)]
    c.close()


# ------------------------------------------------------------------ 5. nothing is disturbed
def test_add_and_fetch_disturb_no_view_counter_or_timing():
    w = _world("syn")
    bases, off, r = _syn_run()
    lo, hi = 0, 500
    pb, po = _part(bases, off, lo, hi)
    batch = dict(bases=pb, offsets=po, quals=None, names=np.frombuffer(b"".join(b"q%d" % i for i in range(hi - lo)), np.uint8),
                 name_off=np.cumsum([0] + [len(b"q%d" % i) for i in range(hi - lo)]).astype("<u8"))
    a = w.aligner(capi.CI_OPTS)
    c = capi.Coverage(a, 3)
    # before any run an add fails as a fetch does
    e_add, e_fetch = _raises(c.add), _raises(a.fetch)
    assert (e_add.code, str(e_add)) == (e_fetch.code, str(e_fetch))
    a.upload_reads(batch)
    a.run()
    views = (a.fetch(copy=False), a.fetch_cigars(copy=False), a.fetch_bam(copy=False))
    fields = [("offsets", "alns", "ops"), ("offsets", "alns", "digests", "cigar"), ("data", "read_rec_off")]
    snap = [[getattr(v, f).copy() for f in fs] for v, fs in zip(views, fields)]
    counters, timings = a.counters(), a.timings()
    info = c.add()
    got = [c.fetch(k, 0, 1) for k in range(4)]
    c.depth(0, 0, 100, 1000)
    assert info["n_reads"] == hi - lo and info["add_ms"] > 0 and got[0].fetch_ms > 0
    assert np.array_equal(a.counters(), counters) and a.timings() == timings
    for v, fs, s in zip(views, fields, snap):
        for f, x in zip(fs, s):
            assert np.array_equal(getattr(v, f), x), f
    again = (a.fetch(), a.fetch_cigars(), a.fetch_bam())
    for v, fs, s in zip(again, fields, snap):
        for f, x in zip(fs, s):
            assert np.array_equal(getattr(v, f), x), f
    assert np.array_equal(a.counters(), counters)
    a0, a1 = int(r.offsets[lo]), int(r.offsets[hi])
    dig, words = cc.expected_alignments(r.alns[a0:a1], r.ops)
    sub = cv.Expect(w.t, 3)
    sub.add((r.offsets[lo: hi + 1] - r.offsets[lo]).astype("<u8"), r.alns[a0:a1], dig, words)
    for k in range(4):
        cv.check_result(got[k], sub, k, 0, 1)
    # after the aligner's next upload the run is gone, for the add as for the fetches; what was added stays
    a.upload(pb, po)
    e_add, e_fetch = _raises(c.add), _raises(a.fetch)
    assert (e_add.code, str(e_add)) == (e_fetch.code, str(e_fetch))
    cv.check_result(c.fetch(1, 0, 1), sub, 1, 0, 1)
    # the free order: the tracks before their aligner; a second close is harmless
    c.close()
    c.close()
    a.close()


# ------------------------------------------------------------------ 6. the file driver
@contextlib.contextmanager
def _knobs(**kv):
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def test_file_driver_writes_the_tracks(tmp_path):
    bases, off, r = _syn_run()
    w = _world("syn")
    n = len(off) - 1
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(b"".join(b"@r%d\n" % i + bytes(bases[int(off[i]): int(off[i + 1])]) + b"\n+\n" + b"I" * int(off[i + 1] - off[i]) + b"\n" for i in range(n)))
    a = w.aligner(capi.CI_OPTS)
    a2 = w.aligner(capi.CI_OPTS)
    names = qc.sq_names(w.t)

    def run(tag, fmt, aligners=a, **knobs):
        out = tmp_path / tag
        with _knobs(**knobs):
            capi.align_files(aligners, [fq], out, fmt, batch_reads=700, n_threads=4)   # 700 does not divide 4000
        tracks = {p.name[len(tag) + 5: -9]: p.read_text() for p in tmp_path.glob(tag + ".cov.*.bedgraph")}
        return out.read_bytes(), tracks

    plain, none = run("sam_plain", capi.FMT_SAM)
    assert none == {}
    sam = str(tmp_path / "sam_plain")
    for mode, flags in ((1, 0), (2, cv.STRANDED), (3, cv.STRANDED | cv.MULTI)):
        # what the run's own SAM output holds, counted line by line ...
        depth = cv.sam_depth(sam, w.t, flags)
        want = {name: cv.bedgraph(names, depth[k]) for k, name in enumerate(cv.track_names(flags))}
        # ... and the expectation from the oracle says the same
        exp = _syn_expect(flags)
        assert want == {name: cv.bedgraph(names, [exp.depth(k, 0)]) for k, name in enumerate(cv.track_names(flags))}
        assert all(len(x) > 1000 for x in want.values())
        for n_aligners in (1, 2):
            tag = "cov%d_%d" % (mode, n_aligners)
            got, tracks = run(tag, capi.FMT_SAM, aligners=a if n_aligners == 1 else [a, a2], THM_COVERAGE=mode)
            assert got == plain and tracks == want, tag
    # a device-encoded BAM with the count tables beside: the same tracks, the same file as without the knob
    bam_plain, _ = run("bam_plain", capi.FMT_BAM, THM_BAM_DEVICE=1)
    got, tracks = run("bam_cov", capi.FMT_BAM, THM_BAM_DEVICE=1, THM_COVERAGE=3, THM_QUANT=1)
    assert got == bam_plain and tracks == want and (tmp_path / "bam_cov.genes.tsv").exists()
    # to standard output there is nowhere to put the tracks
    with _knobs(THM_COVERAGE=1):
        e = _raises(lambda: capi.align_files(a, [fq], "-", capi.FMT_SAM, batch_reads=700, n_threads=4))
    assert e.code == capi.ERR_INVALID_ARG and "THM_COVERAGE" in str(e) and "needs an output file" in str(e)
    a.close()
    a2.close()
