"""-m gpu: the gene and junction count tables of a run, built on the device (kernels_quant.hip, thm_quant).  Every case
compares the three results of a fetch -- totals, gene rows, junction rows -- with the expectation of tests/quant_common.py,
which is written from the contract in include/thermite_io.h and counts the oracle's alignments (or a view made by hand)."""
import contextlib
import os

import numpy as np
import pytest

import bam_common as bc
import quant_common as qc
from gpu_common import World
from thermite_amd import capi

pytestmark = pytest.mark.gpu

_memo = {}
KNOBS = ("THM_QUANT", "THM_BAM_SORT", "THM_BAM_INDEX", "THM_BAM_DEVICE", "THM_FASTQ_DEVICE")


def _world(key, wide=False):
    if (key, wide) not in _memo:
        t = {"test_ref": lambda: bc.tables("test_ref"), "syn": qc.syn_tables, "big": qc.big_gene_tables}[key]()
        _memo[(key, wide)] = World(t, wide)
    return _memo[(key, wide)]


def _syn_run():
    """(bases, offsets, the oracle's result, the expected tables) of the synthetic run; the oracle runs once"""
    if "run" not in _memo:
        w = _world("syn")
        bases, off = qc.syn_reads(w.t)
        r = w.oix.align_batch(bases, off, capi.CI_OPTS, n_threads=8)
        assert r.counters[15] == 0
        _memo["run"] = (bases, off, r, qc.from_oracle(w.t, r))
    return _memo["run"]


def _part(bases, off, lo, hi):
    b0 = int(off[lo])
    return bases[b0: int(off[hi])], (off[lo: hi + 1] - off[lo]).astype("<u8")


def _add_reads(a, q, bases, off):
    a.upload(bases, off)
    a.run()
    return q.add()


def _raises(f):
    with pytest.raises(capi.ThermiteError) as e:
        f()
    return e.value


# ------------------------------------------------------------------ 1. config 1 through the aligner
def test_config_1_gives_the_hand_tables():
    w = _world("test_ref")
    rs = bc.read_set("test_query", w.t)
    b = bc.batch_of(rs)
    a = w.aligner(rs["opts"])
    q = capi.Quant(a)
    info = _add_reads(a, q, b["bases"], b["offsets"])
    res = q.fetch()
    qc.assert_golden(w.t, qc.of_result(res))
    assert {k: info[k] for k in qc.TOTAL_NAMES} == qc.GOLDEN_TOTALS and info["n_junctions"] == 5 and info["held_bytes"] > 0
    q.close()
    a.close()


def test_create_takes_the_bam_layers_precondition_on_names():
    w = _world("test_ref")
    rs = bc.read_set("test_query", w.t)
    t = {k: v for k, v in w.t.items() if k not in ("names", "tx_ids", "gene_ids", "gene_names")}
    ix = capi.Index(t)
    a = capi.Aligner(ix, rs["opts"])
    a.upload_reads(bc.batch_of(rs))
    a.run()
    e_bam = _raises(a.fetch_bam)
    e = _raises(lambda: capi.Quant(a))
    assert (e.code, str(e)) == (e_bam.code, str(e_bam)) and e.code == capi.ERR_INVALID_ARG and "names" in str(e)
    a.close()
    ix.close()


# ------------------------------------------------------------------ 2. the synthetic run
@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
def test_synthetic_run_against_the_expectation(wide):
    bases, off, r, exp = _syn_run()
    w = _world("syn", wide)
    a = w.aligner(capi.CI_OPTS)
    q = capi.Quant(a)
    a.reset_counters()
    c0 = a.counters()
    info = _add_reads(a, q, bases, off)
    c = a.counters() - c0
    got = qc.of_result(q.fetch())
    qc.assert_tables_equal(got, exp)
    qc.check_invariants(got)
    tot = got["totals"]
    assert {k: info[k] for k in qc.TOTAL_NAMES} == tot and info["n_junctions"] == len(exp["junctions"]) >= 200
    g = got["genes"]
    assert int(c[3]) == tot["n_alns"] and int(c[0]) == tot["n_reads"] and int(c[2]) == tot["n_unmapped_reads"]
    assert int(c[4]) == int(g["exonic_unique"].sum() + g["exonic_multi"].sum())
    assert int(c[5]) == int(g["intronic_unique"].sum() + g["intronic_multi"].sum())
    assert int(c[6]) == tot["n_intergenic_unique"] + tot["n_intergenic_multi"]
    q.close()
    a.close()


# ------------------------------------------------------------------ 3. batching and order
def test_batches_in_any_cut_and_order_give_the_same_bytes():
    bases, off, r, exp = _syn_run()
    w = _world("syn")
    n = len(off) - 1
    cuts = [0, 1, 64, 128, 193, n]   # batches of 1, 63, 64, 65 reads and the rest
    a = w.aligner(capi.CI_OPTS)
    for order in (range(5), reversed(range(5))):
        q = capi.Quant(a)
        for k in order:
            _add_reads(a, q, *_part(bases, off, cuts[k], cuts[k + 1]))
        assert qc.pack(qc.of_result(q.fetch())) == qc.pack(exp)
        q.close()
    # one batch added 20 times: the table and the memory stay, the counts are 20-fold
    for k in (0, 3):
        q = capi.Quant(a)
        first = _add_reads(a, q, *_part(bases, off, cuts[k], cuts[k + 1]))
        once = qc.of_result(q.fetch())
        for _ in range(19):
            info = q.add()
            assert (info["n_junctions"], info["held_bytes"]) == (first["n_junctions"], first["held_bytes"])
            assert {f: info[f] for f in qc.TOTAL_NAMES} == {f: first[f] for f in qc.TOTAL_NAMES}
        qc.assert_tables_equal(qc.of_result(q.fetch()), qc.scale_tables(once, 20), "20 adds of batch %d" % k)
        if k == 3:
            assert first["n_junctions"] > 0 and first["n_alns"] >= 60
        q.close()
    a.close()


# ------------------------------------------------------------------ 4. the shapes of add_view
SHAPES = ["empty", "no_alignments", "one_read_5000", "unique_70000", "forty_introns", "long_run", "both_strands", "later_overhang"]


@pytest.mark.parametrize("name", SHAPES)
def test_add_view_shapes(name):
    w = _world("syn")
    q = capi.Quant(w.a)
    exp = None
    for view in qc.shape_cases(w.t)[name]:
        info = q.add_view(*view)
        one = qc.expected_tables(w.t, *view)
        assert {k: info[k] for k in qc.TOTAL_NAMES} == one["totals"]
        exp = one if exp is None else qc.add_tables(exp, one)
        qc.assert_tables_equal(qc.of_result(q.fetch()), exp, name)
    assert info["n_junctions"] == len(exp["junctions"])
    if name == "one_read_5000":
        j = exp["junctions"]
        assert len(j) == 1 and int(j["n_multi"][0]) == 5000 and int(j["n_unique"][0]) == 0
    if name == "unique_70000":
        assert int(exp["junctions"]["n_unique"][0]) == 70000 > 0xFFFF and int(exp["genes"]["exonic_unique"].max()) == 70000
    if name == "later_overhang":
        assert int(exp["junctions"]["max_overhang"][0]) == 15
    q.close()


def test_add_view_on_a_gene_table_beyond_any_lds_histogram():
    w = _world("big")
    view = qc.big_gene_view(w.t)
    exp = qc.expected_tables(w.t, *view)
    assert len(exp["genes"]) * 4 == 48000
    q = capi.Quant(w.a)
    q.add_view(*view)
    qc.assert_tables_equal(qc.of_result(q.fetch()), exp)
    q.add_view(*view)
    qc.assert_tables_equal(qc.of_result(q.fetch()), qc.scale_tables(exp, 2))
    q.close()


def test_add_view_refuses_a_bad_view_and_adds_nothing():
    w = _world("syn")
    q = capi.Quant(w.a)
    good = qc.shape_cases(w.t)["both_strands"][0]
    q.add_view(*good)
    before = qc.pack(qc.of_result(q.fetch()))
    off, alns, dig, words = good
    bad = alns.copy()
    bad["tx_or_gene_idx"][1] = len(w.t["txs"])
    e = _raises(lambda: q.add_view(off, bad, dig, words))
    assert e.code == capi.ERR_INVALID_ARG and "alignment 1" in str(e) and "tx_or_gene_idx" in str(e)
    bad = alns.copy()
    bad["ref_id"][2] = len(w.t["refs"])
    assert _raises(lambda: q.add_view(off, bad, dig, words)).code == capi.ERR_INVALID_ARG
    bad = dig.copy()
    bad["cigar_off"][0] = len(words) - 1
    assert "alignment 0" in str(_raises(lambda: q.add_view(off, alns, bad, words)))
    assert _raises(lambda: q.add_view(off[::-1].copy(), alns, dig, words)).code == capi.ERR_INVALID_ARG
    assert qc.pack(qc.of_result(q.fetch())) == before
    q.close()


# ------------------------------------------------------------------ 5. nothing is disturbed
def test_add_disturbs_no_view_counter_or_timing():
    w = _world("syn")
    bases, off, r, exp = _syn_run()
    lo, hi = 0, 500
    pb, po = _part(bases, off, lo, hi)
    batch = dict(bases=pb, offsets=po, quals=None, names=np.frombuffer(b"".join(b"q%d" % i for i in range(hi - lo)), np.uint8),
                 name_off=np.cumsum([0] + [len(b"q%d" % i) for i in range(hi - lo)]).astype("<u8"))
    a = w.aligner(capi.CI_OPTS)
    q = capi.Quant(a)
    # before any run an add fails as a fetch does
    e_add, e_fetch = _raises(q.add), _raises(a.fetch)
    assert (e_add.code, str(e_add)) == (e_fetch.code, str(e_fetch))
    a.upload_reads(batch)
    a.run()
    views = (a.fetch(copy=False), a.fetch_cigars(copy=False), a.fetch_bam(copy=False))
    fields = [("offsets", "alns", "ops"), ("offsets", "alns", "digests", "cigar"), ("data", "read_rec_off")]
    snap = [[getattr(v, f).copy() for f in fs] for v, fs in zip(views, fields)]
    counters, timings = a.counters(), a.timings()
    info = q.add()
    assert info["n_reads"] == hi - lo and info["add_ms"] > 0
    assert np.array_equal(a.counters(), counters) and a.timings() == timings
    for v, fs, s in zip(views, fields, snap):
        for f, x in zip(fs, s):
            assert np.array_equal(getattr(v, f), x), f
    again = (a.fetch(), a.fetch_cigars(), a.fetch_bam())
    for v, fs, s in zip(again, fields, snap):
        for f, x in zip(fs, s):
            assert np.array_equal(getattr(v, f), x), f
    assert np.array_equal(a.counters(), counters)
    one = qc.of_result(q.fetch())
    sub = qc.expected_tables(w.t, *_oracle_part(r, lo, hi))
    qc.assert_tables_equal(one, sub)
    # an add between two fetches, and a second add of the same run
    q.add()
    qc.assert_tables_equal(qc.of_result(q.fetch()), qc.scale_tables(sub, 2))
    # reset empties everything; the object goes on
    q.reset()
    z = qc.of_result(q.fetch())
    assert len(z["junctions"]) == 0 and not any(z["totals"].values()) and not any(z["genes"][f].any() for f in qc.GENE_DT.names)
    q.add()
    qc.assert_tables_equal(qc.of_result(q.fetch()), sub)
    # after the aligner's next upload the run is gone, for the add as for the fetches
    a.upload(pb, po)
    e_add, e_fetch = _raises(q.add), _raises(a.fetch)
    assert (e_add.code, str(e_add)) == (e_fetch.code, str(e_fetch))
    qc.assert_tables_equal(qc.of_result(q.fetch()), sub)
    # the free order: the tables before their aligner; a second close is harmless
    q.close()
    q.close()
    a.close()


def _oracle_part(r, lo, hi):
    """reads [lo, hi) of an oracle result as a view (offsets, records, digests, words)"""
    import cigar_common as cc
    a0, a1 = int(r.offsets[lo]), int(r.offsets[hi])
    dig, words = cc.expected_alignments(r.alns[a0:a1], r.ops)
    return (r.offsets[lo: hi + 1] - r.offsets[lo]).astype("<u8"), r.alns[a0:a1], dig, words


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


def test_file_driver_writes_both_tables(tmp_path):
    bases, off, r, exp = _syn_run()
    w = _world("syn")
    n = len(off) - 1
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(b"".join(b"@r%d\n" % i + bytes(bases[int(off[i]): int(off[i + 1])]) + b"\n+\n" + b"I" * int(off[i + 1] - off[i]) + b"\n" for i in range(n)))
    a = w.aligner(capi.CI_OPTS)
    a2 = w.aligner(capi.CI_OPTS)
    want = qc.tsv_of(w.t, exp)

    def run(tag, fmt, aligners=a, **knobs):
        out = tmp_path / tag
        with _knobs(**knobs):
            capi.align_files(aligners, [fq], out, fmt, batch_reads=700, n_threads=4)   # 700 does not divide 4000
        g, j = tmp_path / (tag + ".genes.tsv"), tmp_path / (tag + ".junctions.tsv")
        return out.read_bytes(), (g.read_text(), j.read_text()) if g.exists() and j.exists() else None

    modes = [("sam", capi.FMT_SAM, {}), ("bam", capi.FMT_BAM, dict(THM_BAM_DEVICE=1)), ("sorted", capi.FMT_BAM, dict(THM_BAM_SORT=1))]
    for tag, fmt, knobs in modes:
        plain, none = run(tag + "_plain", fmt, **knobs)
        counted, tables = run(tag + "_quant", fmt, THM_QUANT=1, **knobs)
        assert none is None and counted == plain, tag
        assert tables == want, tag
    # the path that does not go through the oracle: the SAM file's own tags, positions and CIGARs
    genes, rows = qc.count_sam(str(tmp_path / "sam_plain"), w.t)
    assert qc.tsv_of_sam_counts(w.t, genes, rows) == want
    assert want[1].count("\n") - 1 >= 200
    # two aligners on the one device: the same files
    both, tables = run("two", capi.FMT_SAM, aligners=[a, a2], THM_QUANT=1)
    assert tables == want and both == (tmp_path / "sam_plain").read_bytes()
    # to standard output there is nowhere to put the tables
    with _knobs(THM_QUANT=1):
        e = _raises(lambda: capi.align_files(a, [fq], "-", capi.FMT_SAM, batch_reads=700, n_threads=4))
    assert e.code == capi.ERR_INVALID_ARG and "THM_QUANT" in str(e)
    a.close()
    a2.close()
