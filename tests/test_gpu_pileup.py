"""-m gpu: the per-base allele counts of a run, built on the device (kernels_pileup.hip, thm_pileup).  Every case compares
what a fetch or a window returns -- rows of sites, the view's counts, totals -- with the expectation of
tests/pileup_common.py, which is written from the contract in include/thermite_io.h and walks the oracle's alignments (or
a view made by hand) into per-base arrays; the file driver's table is compared with the line-by-line count of the run's
own SAM output."""
import contextlib
import os
import re

import numpy as np
import pytest

import bam_common as bc
import cigar_common as cc
import pileup_common as pc
import quant_common as qc
from gpu_common import World
from thermite_amd import capi

pytestmark = pytest.mark.gpu

_memo = {}
KNOBS = ("THM_PILEUP", "THM_PILEUP_MIN_ALT", "THM_COVERAGE", "THM_QUANT", "THM_BAM_SORT", "THM_BAM_INDEX", "THM_BAM_DEVICE", "THM_FASTQ_DEVICE")
CHUNK, GROUP, TILE = capi.PILE_CHUNK, capi.PILE_GROUP, capi.COV_TILE
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _world(key, wide=False):
    if (key, wide) not in _memo:
        t = {"test_ref": lambda: bc.tables("test_ref"), "syn": qc.syn_tables, "shape": pc.shape_tables}[key]()
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
        bases, off, r = _syn_run()
        _memo[("exp", flags)] = pc.from_oracle(_world("syn").t, flags, r, bases, off)
    return _memo[("exp", flags)]


def _shapes():
    if "shapes" not in _memo:
        _memo["shapes"] = pc.shape_cases(_world("shape").t, CHUNK, GROUP, TILE)
    return _memo["shapes"]


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
    return {k: info[k] for k in pc.TOTAL_NAMES}


def _check_all(c, exp, what="", min_alts=(1,)):
    """all contigs together and contig by contig, at every threshold"""
    n_sq = len(exp.lens)
    for m in min_alts:
        pc.check_fetch(c.fetch(0, n_sq, m), exp, 0, n_sq, m, what)
        for s in range(n_sq):
            pc.check_fetch(c.fetch(s, 1, m), exp, s, 1, m, "%s contig %d" % (what, s))


def _pack(c, n_sq, windows=()):
    return b"".join(c.fetch(0, n_sq, m).sites.tobytes() for m in (1, 2)) + b"".join(c.window(*w).sites.tobytes() for w in windows)


# ------------------------------------------------------------------ 1. config 1 through the aligner
@pytest.mark.parametrize("flags", [0, pc.MULTI])
def test_config_1_gives_the_hand_rows(flags):
    w = _world("test_ref")
    rs = bc.read_set("test_query", w.t)
    b = bc.batch_of(rs)
    a = w.aligner(rs["opts"])
    c = capi.Pileup(a, flags)
    info = _add_reads(a, c, b["bases"], b["offsets"])
    res = c.fetch(0, 4, 1)
    names = qc.sq_names(w.t)
    want = pc.sam_pileup(os.path.join(DATA, "test_query.sam"), pc.parse_fasta_text(os.path.join(DATA, "data", "test_ref.fasta")), names, multi=bool(flags))
    assert pc.rows_as_tuples(names, res.sites) == want and len(want) == 2
    assert [(int(r["ref_id"]), int(r["pos"]), chr(r["ref_base"]), int(r["depth"])) for r in res.sites] == [(2, 21, "T", 4), (3, 20, "T", 2)]
    assert res.sites["cnt"].tolist() == [[0, 1, 0, 3, 0], [1, 0, 0, 1, 0]]
    exp = pc.Expect(w.t, flags)
    exp.add(*pc.sam_view(os.path.join(DATA, "test_query.sam"), w.t))
    assert _batch_totals(info) == exp.totals == res.totals and info["n_events"] == 2 and info["held_bytes"] > 0
    for s, n in enumerate(exp.lens):
        pc.check_window(c.window(s, 0, n), exp, s, 0, n, "config 1")
    c.close()
    a.close()


# ------------------------------------------------------------------ 2. the synthetic run
@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
def test_synthetic_run_against_the_expectation(wide):
    bases, off, r = _syn_run()
    w = _world("syn", wide)
    a = w.aligner(capi.CI_OPTS)
    n = pc.contig_lens(w.t)[0]
    dig, _ = cc.expected_alignments(r.alns, r.ops)
    n_alns = np.diff(r.offsets.astype(np.int64))
    for flags in (0, pc.MULTI):
        exp = _syn_expect(flags)
        c = capi.Pileup(a, flags)
        info = _add_reads(a, c, bases, off) if flags == 0 else c.add()
        assert _batch_totals(info) == exp.totals and info["n_events"] == exp.n_events()
        _check_all(c, exp, "flags %d" % flags, (1, 2, 3))
        # windows that start mid-tile, end on the contig's last base, hold one base: the invariant holds on every row
        first = int(exp.rows()["pos"][0])
        for start, m in ((0, 1), (TILE + 17, 3 * TILE), (n - 5000, 5000), (n - 1, 1), (TILE - 1, 2), (first, 300)):
            pc.check_window(c.window(0, start, m), exp, 0, start, m, "flags %d" % flags)
        # against the oracle: over ACGTN a mismatch is a substitution
        used = np.repeat(n_alns == 1, n_alns) if flags == 0 else np.ones(len(dig), bool)
        assert info["n_mismatches"] == int(dig["n_subst"][used].sum()) and info["n_used_alns"] == int(used.sum())
        c.close()
    a.close()


# ------------------------------------------------------------------ 3. the shapes of add_view
SHAPES = ["empty", "no_alignments", "perfect", "contig_ends", "next_to_S", "next_to_I", "next_to_D", "next_to_N", "ins_behind_s_and_n", "d_next_to_n",
          "reverse_ends", "lengths", "forty_introns", "hot_same_mismatch", "hot_every_kind", "tile_edges", "letters", "long_run", "multi", "later_add"]


def test_the_shape_list_is_complete():
    assert sorted(SHAPES) == sorted(_shapes())


@pytest.mark.parametrize("name", SHAPES)
def test_add_view_shapes(name):
    w = _world("shape")
    for flags in (0, pc.MULTI):
        c = capi.Pileup(w.a, flags)
        exp = pc.Expect(w.t, flags)
        for view in _shapes()[name]:
            info = c.add_view(*view)
            assert _batch_totals(info) == exp.add(*view), (name, flags)
            assert info["n_events"] == exp.n_events()
            _check_all(c, exp, "%s flags %d" % (name, flags), (1, 2, 3))
        for s, start, n in pc.shape_windows(TILE):
            pc.check_window(c.window(s, start, n), exp, s, start, n, "%s flags %d" % (name, flags))
        c.close()


# ------------------------------------------------------------------ 4. merging and filtering
def test_batches_in_any_cut_and_order_give_the_same_bytes():
    bases, off, r = _syn_run()
    w = _world("syn")
    exp = _syn_expect(pc.MULTI)
    n, m = len(off) - 1, pc.contig_lens(w.t)[0]
    windows = [(0, 0, 3 * TILE + 5), (0, m - 2000, 2000)]
    want = b"".join(exp.rows(min_alt=k).tobytes() for k in (1, 2)) + b"".join(exp.window(*x).tobytes() for x in windows)
    cuts = [0, 1, 64, 128, 193, n]   # batches of 1, 63, 64, 65 reads and the rest
    a = w.aligner(capi.CI_OPTS)
    c = capi.Pileup(a, pc.MULTI)
    for order in (range(5), reversed(range(5))):
        for k in order:
            info = _add_reads(a, c, *_part(bases, off, cuts[k], cuts[k + 1]))
        assert _pack(c, 1, windows) == want
        assert c.fetch(0, 1, 1).totals == exp.totals and info["n_events"] == exp.n_events()
        # reset empties the object, which goes on
        c.reset()
        z = c.fetch(0, 1, 1)
        assert len(z.sites) == 0 and z.n_events == 0 and z.totals == pc.Expect(w.t, 0).totals and not c.window(0, 0, 4000).sites["depth"].any()
    c.close()
    a.close()


def test_the_same_event_in_two_batches_is_one_row_and_a_run_twice_doubles_every_count():
    bases, off, r = _syn_run()
    w = _world("syn")
    a = w.aligner(capi.CI_OPTS)
    c = capi.Pileup(a, 0)
    first = _add_reads(a, c, bases, off)
    second = c.add()
    exp = _syn_expect(0)
    assert second["n_events"] == first["n_events"] == exp.n_events() and _batch_totals(second) == _batch_totals(first)
    _check_all(c, exp.scaled(2), "twice", (1, 2, 3))
    n = pc.contig_lens(w.t)[0]
    pc.check_window(c.window(0, n - 3 * TILE, 3 * TILE), exp.scaled(2), 0, n - 3 * TILE, 3 * TILE, "twice")
    # an add whose rows the table all holds allocates nothing (the fetches above have made their scratch by now)
    third = c.add()
    fourth = c.add()
    assert fourth["held_bytes"] == third["held_bytes"] and fourth["n_events"] == third["n_events"] == first["n_events"]
    assert third["held_bytes"] >= second["held_bytes"]
    c.close()
    a.close()
    # by hand: one mismatch added in two views is one row with the sum
    ws = _world("shape")
    c = capi.Pileup(ws.a, 0)
    view = _shapes()["hot_same_mismatch"][0]
    assert c.add_view(*view)["n_events"] == 1 and c.add_view(*view)["n_events"] == 1
    rows = c.fetch(0, 3, 1).sites
    assert len(rows) == 1 and int(rows[0]["depth"]) == 10000 and sorted(rows[0]["cnt"].tolist()) == [0, 0, 0, 0, 10000]
    c.close()


# ------------------------------------------------------------------ 5. refusals
def test_create_and_the_calls_refuse_what_they_must():
    w = _world("test_ref")
    rs = bc.read_set("test_query", w.t)
    # the names precondition of the BAM layer, with its message
    t = {k: v for k, v in w.t.items() if k not in ("names", "tx_ids", "gene_ids", "gene_names")}
    ix = capi.Index(t)
    a = capi.Aligner(ix, rs["opts"])
    a.upload_reads(bc.batch_of(rs))
    a.run()
    e_bam = _raises(a.fetch_bam)
    e = _raises(lambda: capi.Pileup(a))
    assert (e.code, str(e)) == (e_bam.code, str(e_bam)) and e.code == capi.ERR_INVALID_ARG and "names" in str(e)
    a.close()
    ix.close()
    a = w.aligner(rs["opts"])
    assert _raises(lambda: capi.Pileup(a, 2)).code == capi.ERR_INVALID_ARG
    # a cap one below the arrays: the message holds both numbers; the arrays alone fit their size
    e = _raises(lambda: capi.Pileup(a, 0, 1))
    assert e.code == capi.ERR_OOM
    need = int(re.search(r"needs (\d+) bytes, the cap is 1\b", str(e)).group(1))
    assert need >= 4 * sum(pc.contig_lens(w.t))
    e = _raises(lambda: capi.Pileup(a, 0, need - 1))
    assert e.code == capi.ERR_OOM and str(need) in str(e) and str(need - 1) in str(e)
    c = capi.Pileup(a, 0, need)
    for f in (lambda: c.fetch(0, 4, 0), lambda: c.fetch(3, 2, 1), lambda: c.fetch(5, 0, 1), lambda: c.window(4, 0, 1), lambda: c.window(1, 0, 13),
              lambda: c.window(1, 12, 1)):
        assert _raises(f).code == capi.ERR_INVALID_ARG
    assert len(c.fetch(4, 0, 1).sites) == 0 and len(c.window(1, 12, 0).sites) == 0
    c.close()
    a.close()
    ws = _world("shape")
    c = capi.Pileup(ws.a, 0)
    e = _raises(lambda: c.window(0, 0, (1 << 20) + 1))
    assert e.code == capi.ERR_INVALID_ARG and "2^20" in str(e)
    c.close()


def test_a_table_over_the_cap_is_refused_and_the_next_fetch_is_unchanged():
    w = _world("shape")
    probe = capi.Pileup(w.a, 0)
    one, two = _shapes()["later_add"][0], _shapes()["lengths"][0]
    n_one = probe.add_view(*one)["n_events"]
    n_both = probe.add_view(*two)["n_events"]
    probe.close()
    assert n_both > n_one + 100
    arrays = int(re.search(r"needs (\d+) bytes", str(_raises(lambda: capi.Pileup(w.a, 0, 1)))).group(1))
    c = capi.Pileup(w.a, 0, arrays + 12 * n_both - 1)      # the arrays, the first table, not the merged one
    c.add_view(*one)
    before = _pack(c, 3, [(0, 8990, 200)]), c.fetch(0, 3, 1).totals
    e = _raises(lambda: c.add_view(*two))
    assert e.code == capi.ERR_OOM and str(arrays + 12 * n_both) in str(e) and str(arrays + 12 * n_both - 1) in str(e)
    assert (_pack(c, 3, [(0, 8990, 200)]), c.fetch(0, 3, 1).totals) == before
    c.close()
    c = capi.Pileup(w.a, 0, arrays + 12 * n_both)          # one byte more and it fits
    c.add_view(*one)
    assert c.add_view(*two)["n_events"] == n_both
    c.close()


def test_a_bad_view_is_refused_and_the_next_fetch_is_unchanged():
    w = _world("shape")
    c = capi.Pileup(w.a, pc.MULTI)
    good = _shapes()["later_add"][0]
    c.add_view(*good)
    before = _pack(c, 3, [(0, 8990, 200)]), c.fetch(0, 3, 1).totals
    for name, bad in pc.bad_views(w.t).items():
        e = _raises(lambda: c.add_view(*bad))
        assert e.code == capi.ERR_INVALID_ARG and "alignment 1" in str(e), (name, str(e))
    # digests that understate ref_len pass the host's check: the device's pass finds the walk's end
    off, alns, dig, words, bases, base_off = pc.bad_views(w.t)["past_the_contig"]
    lie = dig.copy()
    lie["ref_len"][1] = 50
    e = _raises(lambda: c.add_view(off, alns, lie, words, bases, base_off))
    assert e.code == capi.ERR_INVALID_ARG and "alignment 1" in str(e) and "contig" in str(e)
    # base_off that does not start at 0, or descends
    down = base_off.copy()
    down[1] = down[2] + 1
    for bo in (base_off + 1, down):
        e = _raises(lambda: c.add_view(off, alns, dig, words, bases, bo))
        assert e.code == capi.ERR_INVALID_ARG and "base_off" in str(e)
    assert (_pack(c, 3, [(0, 8990, 200)]), c.fetch(0, 3, 1).totals) == before
    # the alignment that ends exactly at the contig's length is taken
    fit = words.copy()
    fit[-1] -= 1 << 4
    dig2 = dig.copy()
    dig2["ref_len"][1] -= 1
    c.add_view(off, alns, dig2, fit, bases[:-1], np.concatenate([base_off[:-1], base_off[-1:] - 1]))
    assert c.window(1, 999, 1).sites["depth"].tolist() == [1]
    c.close()


# ------------------------------------------------------------------ 6. nothing is disturbed
def test_add_fetch_and_window_disturb_no_view_counter_or_timing():
    w = _world("syn")
    bases, off, r = _syn_run()
    lo, hi = 0, 500
    pb, po = _part(bases, off, lo, hi)
    batch = dict(bases=pb, offsets=po, quals=None, names=np.frombuffer(b"".join(b"q%d" % i for i in range(hi - lo)), np.uint8),
                 name_off=np.cumsum([0] + [len(b"q%d" % i) for i in range(hi - lo)]).astype("<u8"))
    a = w.aligner(capi.CI_OPTS)
    c = capi.Pileup(a, pc.MULTI)
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
    got = c.fetch(0, 1, 1)
    win = c.window(0, 100, 1000)
    assert info["n_reads"] == hi - lo and info["add_ms"] > 0 and got.fetch_ms > 0 and win.fetch_ms > 0
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
    sub = pc.Expect(w.t, pc.MULTI)
    sub.add((r.offsets[lo: hi + 1] - r.offsets[lo]).astype("<u8"), r.alns[a0:a1], dig, words, pb, po)
    pc.check_fetch(got, sub, 0, 1, 1)
    pc.check_window(win, sub, 0, 100, 1000)
    # after the aligner's next upload the run is gone, for the add as for the fetches; what was added stays
    a.upload(pb, po)
    e_add, e_fetch = _raises(c.add), _raises(a.fetch)
    assert (e_add.code, str(e_add)) == (e_fetch.code, str(e_fetch))
    pc.check_fetch(c.fetch(0, 1, 2), sub, 0, 1, 2)
    # the free order: the counts before their aligner; a second close is harmless
    c.close()
    c.close()
    a.close()


# ------------------------------------------------------------------ 7. the file driver
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


def test_file_driver_writes_the_sites(tmp_path):
    bases, off, r = _syn_run()
    w = _world("syn")
    n = len(off) - 1
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(b"".join(b"@r%d\n" % i + bytes(bases[int(off[i]): int(off[i + 1])]) + b"\n+\n" + b"I" * int(off[i + 1] - off[i]) + b"\n" for i in range(n)))
    a = w.aligner(capi.CI_OPTS)
    a2 = w.aligner(capi.CI_OPTS)
    names = qc.sq_names(w.t)
    fasta = [(names[s], bytes(seq).decode()) for s, seq in enumerate(pc.contig_seqs(w.t))]

    def run(tag, fmt, aligners=a, **knobs):
        out = tmp_path / tag
        with _knobs(**knobs):
            capi.align_files(aligners, [fq], out, fmt, batch_reads=700, n_threads=4)   # 700 does not divide 4000
        tsv = tmp_path / (tag + ".pileup.tsv")
        return out.read_bytes(), tsv.read_text() if tsv.exists() else None

    plain, none = run("sam_plain", capi.FMT_SAM)
    assert none is None
    sam = str(tmp_path / "sam_plain")
    bam_plain, _ = run("bam_plain", capi.FMT_BAM, THM_BAM_DEVICE=1)

    def beside(tag, *patterns):
        """what a run wrote beside its output: file name behind the tag -> bytes"""
        return {f.name[len(tag):]: f.read_bytes() for pat in patterns for f in sorted(tmp_path.glob(tag + pat))}

    # the tables and tracks of a run that keeps one summary only: what a run with all three on one aligner must write too
    run("quant_alone", capi.FMT_BAM, THM_QUANT=1)
    run("cov_alone", capi.FMT_BAM, THM_COVERAGE=1)
    tables_alone, tracks_alone = beside("quant_alone", ".genes.tsv", ".junctions.tsv"), beside("cov_alone", ".cov.*.bedgraph")
    assert sorted(tables_alone) == [".genes.tsv", ".junctions.tsv"] and tracks_alone and all(tracks_alone.values())
    for mode, flags in ((1, 0), (2, pc.MULTI)):
        for min_alt in (None, 1):
            # what the run's own SAM output holds, counted line by line; the expectation from the oracle says the same
            want = pc.tsv_of_sam(pc.sam_pileup(sam, fasta, names, multi=bool(flags), min_alt=min_alt or 2))
            assert want == pc.tsv(names, _syn_expect(flags).rows(min_alt=min_alt or 2)) and want.count("\n") > 50
            extra = {} if min_alt is None else {"THM_PILEUP_MIN_ALT": min_alt}
            got, tsv = run("pile%d_%s" % (mode, min_alt), capi.FMT_SAM, THM_PILEUP=mode, **extra)
            assert got == plain and tsv == want, (mode, min_alt)
            # a device-encoded BAM with the other tables beside: the same sites, the same file as without the knob
            tag = "bam_pile%d_%s" % (mode, min_alt)
            got, tsv = run(tag, capi.FMT_BAM, THM_BAM_DEVICE=1, THM_PILEUP=mode, THM_COVERAGE=1, THM_QUANT=1, **extra)
            assert got == bam_plain and tsv == want and (tmp_path / (tag + ".genes.tsv")).exists()
            assert beside(tag, ".genes.tsv", ".junctions.tsv") == tables_alone and beside(tag, ".cov.*.bedgraph") == tracks_alone, (mode, min_alt)
    # to standard output there is nowhere to put the table; two aligners' counts are not merged
    with _knobs(THM_PILEUP=1):
        e = _raises(lambda: capi.align_files(a, [fq], "-", capi.FMT_SAM, batch_reads=700, n_threads=4))
        assert e.code == capi.ERR_INVALID_ARG and "THM_PILEUP" in str(e) and "needs an output file" in str(e)
        e = _raises(lambda: capi.align_files([a, a2], [fq], tmp_path / "two", capi.FMT_SAM, batch_reads=700, n_threads=4))
        assert e.code == capi.ERR_INVALID_ARG and "THM_PILEUP takes one aligner" in str(e)
    # a knob that says nothing the driver knows is refused, not read as something else
    for bad in (dict(THM_PILEUP=3), dict(THM_PILEUP=1, THM_PILEUP_MIN_ALT=""), dict(THM_PILEUP=1, THM_PILEUP_MIN_ALT="2x"), dict(THM_PILEUP=1, THM_PILEUP_MIN_ALT=0)):
        with _knobs(**bad):
            e = _raises(lambda: capi.align_files(a, [fq], tmp_path / "bad", capi.FMT_SAM, batch_reads=700, n_threads=4))
            assert e.code == capi.ERR_INVALID_ARG and "THM_PILEUP_MIN_ALT a number" in str(e), bad
    a.close()
    a2.close()
