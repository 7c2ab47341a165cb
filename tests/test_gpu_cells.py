"""-m gpu: the cell-by-gene UMI matrix of a run, built on the device (kernels_cells.hip, thm_cells).  Every case compares
what a fetch returns -- totals, counts, cell rows, entry rows -- with the expectation of tests/cells_common.py, which is
written from the contract in include/thermite_io.h in plain Python over the oracle's alignments (or a view made by hand)
and the reads' names.  Integers throughout: the arrays must be equal."""
import numpy as np
import pytest

import bam_common as bc
import cells_common as cl
import quant_common as qc
from gpu_common import World
from thermite_amd import capi

pytestmark = pytest.mark.gpu

SYN_SEED = 2024   # tests/test_cells_host.py checks what the names of this seed give
_memo = {}


def _world(key, wide=False):
    if (key, wide) not in _memo:
        t = {"test_ref": lambda: bc.tables("test_ref"), "syn": qc.syn_tables, "big": qc.big_gene_tables}[key]()
        _memo[(key, wide)] = World(t, wide)
    return _memo[(key, wide)]


def _syn_run():
    """(batch with names, the oracle's result) of the synthetic run; the oracle runs once"""
    if "run" not in _memo:
        w = _world("syn")
        bases, off = qc.syn_reads(w.t)
        r = w.oix.align_batch(bases, off, capi.CI_OPTS, n_threads=8)
        assert r.counters[15] == 0
        names, name_off = cl.join_names(cl.gen_names(len(off) - 1, SYN_SEED))
        _memo["run"] = (dict(bases=bases, offsets=off, quals=None, names=names, name_off=name_off), r)
    return _memo["run"]


def _syn_expected(flags):
    if ("exp", flags) not in _memo:
        b, r = _syn_run()
        _memo[("exp", flags)] = cl.expected(_world("syn").t, r.offsets, r.alns, None, b["names"], b["name_off"], flags, 16, 12)
    return _memo[("exp", flags)]


def _part(b, lo, hi):
    off, noff = b["offsets"], b["name_off"]
    return dict(bases=b["bases"][int(off[lo]): int(off[hi])], offsets=(off[lo: hi + 1] - off[lo]).astype("<u8"), quals=None,
                names=b["names"][int(noff[lo]): int(noff[hi])], name_off=(noff[lo: hi + 1] - noff[lo]).astype("<u8"))


def _add_reads(a, c, batch):
    a.upload_reads(batch)
    a.run()
    return c.add()


def _raises(f):
    with pytest.raises(capi.ThermiteError) as e:
        f()
    return e.value


def _bytes_of(res):
    return cl.pack_rows(res.cells, res.entries), res.totals, (res.n_molecules, res.n_barcodes, res.n_cells_below)


# ------------------------------------------------------------------ 1. config 1 through the aligner
def test_config_1_through_upload_reads_and_upload_fastq():
    w = _world("test_ref")
    rs = dict(bc.read_set("test_query", w.t))
    rs["names"] = cl.gen_names(len(rs["seqs"]), 11, cb_len=4, umi_len=3, n_barcodes=3, n_umis=2, untagged=0.2)
    b = bc.batch_of(rs)
    r = w.oix.align_batch(b["bases"], b["offsets"], rs["opts"])
    mol, tot = cl.expected(w.t, r.offsets, r.alns, None, b["names"], b["name_off"], 0, 4, 3)
    assert tot["n_counted_reads"] >= 3 and tot["n_unmapped_reads"] == 2 and tot["n_multi_reads"] == 1 and len(mol) >= 2
    a = w.aligner(rs["opts"])
    c = capi.Cells(a, 0, 4, 3)
    info = _add_reads(a, c, b)
    res = c.fetch()
    cl.assert_result(res, mol, tot)
    assert {k: info[k] for k in cl.TOTAL_NAMES} == tot and info["n_molecules"] == len(mol) and info["n_pending"] == 0 and info["held_bytes"] > 0
    assert (res.cb_len, res.umi_len) == (4, 3)
    # the same batch placed by the device's FASTQ parser
    raw = b"".join(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in zip(rs["names"], rs["seqs"], rs["quals"]))
    c2 = capi.Cells(a, 0, 4, 3)
    up = a.upload_fastq(raw)
    assert up["n_reads"] == len(rs["seqs"])
    a.run()
    info2 = c2.add()
    assert {k: info2[k] for k in cl.TOTAL_NAMES} == tot
    assert _bytes_of(c2.fetch()) == _bytes_of(res)
    c.close()
    c2.close()
    a.close()


# ------------------------------------------------------------------ 2. the synthetic run
@pytest.mark.parametrize("flags", [0, capi.CELLS_INTRONIC], ids=["exonic", "intronic"])
@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
def test_synthetic_run_against_the_expectation(wide, flags):
    b, r = _syn_run()
    mol, tot = _syn_expected(flags)
    w = _world("syn", wide)
    a = w.aligner(capi.CI_OPTS)
    c = capi.Cells(a, flags)
    info = _add_reads(a, c, b)
    assert {k: info[k] for k in cl.TOTAL_NAMES} == tot and info["n_molecules"] == len(mol)
    cl.check_invariants(tot, mol)
    for min_umis in (1, 3):
        res = c.fetch(min_umis)
        cl.assert_result(res, mol, tot, min_umis, "min_umis %d" % min_umis)
    assert res.n_cells_below > 0 and len(res.cells) > 0
    c.close()
    a.close()


# ------------------------------------------------------------------ 3. batching and order
def test_batches_in_any_cut_and_order_give_the_same_bytes():
    b, r = _syn_run()
    mol, tot = _syn_expected(0)
    w = _world("syn")
    n = len(b["offsets"]) - 1
    cuts = [0, 1, 64, 128, 193, n]   # batches of 1, 63, 64, 65 reads and the rest
    a = w.aligner(capi.CI_OPTS)
    want = None
    for order in (list(range(5)), list(reversed(range(5)))):
        c = capi.Cells(a)
        so_far_mol, so_far_tot, pending_seen = {}, dict.fromkeys(cl.TOTAL_NAMES, 0), False
        for k in order:
            lo, hi = cuts[k], cuts[k + 1]
            info = _add_reads(a, c, _part(b, lo, hi))
            a0 = int(r.offsets[lo])
            one = cl.expected(w.t, r.offsets[lo: hi + 1] - r.offsets[lo], r.alns[a0: int(r.offsets[hi])], None, *cl.join_names(
                cl.split_names(b["names"], b["name_off"])[lo:hi]), 0, 16, 12)
            assert {f: info[f] for f in cl.TOTAL_NAMES} == one[1]
            so_far_mol, so_far_tot = cl.add_molecules(so_far_mol, one[0]), cl.add_totals(so_far_tot, one[1])
            pending_seen |= info["n_pending"] > 0
            assert info["n_molecules"] >= len(so_far_mol)
            if k == 2:
                # a fetch between adds is a snapshot, and changes nothing after
                cl.assert_result(c.fetch(), so_far_mol, so_far_tot, 1, "snapshot")
                cl.assert_result(c.fetch(2), so_far_mol, so_far_tot, 2, "snapshot")
        if order[0] == 4:
            assert pending_seen   # behind the big batch the small ones wait
        res = c.fetch()
        cl.assert_result(res, mol, tot)
        want = want or _bytes_of(res)
        assert _bytes_of(res) == want and _bytes_of(c.fetch()) == want
        c.close()
    a.close()


# ------------------------------------------------------------------ 4. the same run twice, and reset
def test_the_same_run_twice_doubles_the_reads_and_no_umis():
    b, r = _syn_run()
    mol, tot = _syn_expected(capi.CELLS_INTRONIC)
    w = _world("syn")
    a = w.aligner(capi.CI_OPTS)
    c = capi.Cells(a, capi.CELLS_INTRONIC)
    _add_reads(a, c, b)
    once = c.fetch()
    info = c.add()
    assert info["n_pending"] == 0 and info["n_molecules"] == len(mol)   # as many rows as the table's: merged at once
    twice = c.fetch()
    cl.assert_result(twice, {k: 2 * v for k, v in mol.items()}, {k: 2 * v for k, v in tot.items()})
    assert twice.n_molecules == once.n_molecules == len(mol)
    assert np.array_equal(twice.cells["n_umis"], once.cells["n_umis"]) and np.array_equal(twice.entries["n_umis"], once.entries["n_umis"])
    assert np.array_equal(twice.cells["n_reads"], 2 * once.cells["n_reads"]) and np.array_equal(twice.entries["n_reads"], 2 * once.entries["n_reads"])
    c.reset()
    z = c.fetch()
    assert len(z.cells) == 0 and len(z.entries) == 0 and not any(z.totals.values()) and (z.n_molecules, z.n_barcodes, z.n_cells_below) == (0, 0, 0)
    c.add()
    cl.assert_result(c.fetch(), mol, tot)
    c.close()
    a.close()


# ------------------------------------------------------------------ 5. views made by hand
@pytest.mark.parametrize("cb_len,umi_len", [(1, 1), (16, 16), (16, 12)])
def test_add_view_with_every_class_of_read(cb_len, umi_len):
    w = _world("big")
    offsets, alns, status, names, (dig, words) = cl.class_view(w.t, cb_len, umi_len)
    pool, name_off = cl.join_names(names)
    assert (status != 0).any() and any(offsets[i] == offsets[i + 1] for i in range(1, len(offsets) - 2))
    for flags in (0, capi.CELLS_INTRONIC):
        mol, tot = cl.expected(w.t, offsets, alns, status, pool, name_off, flags, cb_len, umi_len)
        assert all(tot[k] > 0 for k in cl.TOTAL_NAMES if k != "n_intronic_skipped_reads" or not flags), tot
        c = capi.Cells(w.a, flags, cb_len, umi_len)
        info = c.add_view(offsets, alns, dig, words, pool, name_off, status)
        assert {k: info[k] for k in cl.TOTAL_NAMES} == tot and info["n_molecules"] == len(mol)
        for min_umis in (1, 16):
            res = c.fetch(min_umis)
            cl.assert_result(res, mol, tot, min_umis, "%d/%d flags %d" % (cb_len, umi_len, flags))
        # AAAA... sorts first and TTTT... last, its top bits set; the gene field of the key is wide
        first = c.fetch()
        assert int(first.cells["barcode"][0]) == 0 and int(first.cells["barcode"][-1]) == (1 << (2 * cb_len)) - 1
        assert int(first.entries["gene"].max()) == len(w.t["genes"]) - 1 == 11999
        c.close()


# ------------------------------------------------------------------ 6. a table that spans many workgroups, merged more than once
def test_twenty_thousand_reads_in_four_parts():
    w = _world("syn")
    rng = np.random.default_rng(20000)
    n, n_txs = 20000, len(w.t["txs"])
    offsets, alns, dig, words = qc.uniform_view(n, 1, 0, 1000, 0, [(91, "M")])
    alns["tx_or_gene_idx"] = rng.integers(0, n_txs, n)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    bcs = [bytes(acgt[rng.integers(0, 4, 16)]) for _ in range(40)]
    names = [b"s%d_" % i + bcs[int(rng.integers(0, 40))] + b"_" + bytes(acgt[rng.integers(0, 4, 3)]) + b"AAAAAAAAA" for i in range(n)]
    cuts = [0, 4000, 8500, 11000, n]
    c = capi.Cells(w.a)
    mol, tot, infos = {}, dict.fromkeys(cl.TOTAL_NAMES, 0), []
    for lo, hi in zip(cuts, cuts[1:]):
        pool, name_off = cl.join_names(names[lo:hi])
        part = (offsets[lo: hi + 1] - offsets[lo], alns[lo:hi], dig[lo:hi], words)
        infos.append(c.add_view(*part, pool, name_off))
        one = cl.expected(w.t, part[0], part[1], None, pool, name_off, 0, 16, 12)
        mol, tot = cl.add_molecules(mol, one[0]), cl.add_totals(tot, one[1])
    assert 5000 <= len(mol) < tot["n_counted_reads"] == n
    # the first two adds and the last merged, the third waited: its rows lay behind the table's until the fourth
    assert [i["n_pending"] > 0 for i in infos] == [False, False, True, False]
    assert infos[3]["n_molecules"] == len(mol) < infos[2]["n_molecules"] + infos[3]["n_counted_reads"]
    assert infos[2]["n_molecules"] - infos[2]["n_pending"] == infos[1]["n_molecules"]
    median = int(np.median(cl.rows(mol)[0]["n_umis"]))
    for min_umis in (1, median):
        res = c.fetch(min_umis)
        cl.assert_result(res, mol, tot, min_umis)
    assert 0 < len(res.cells) < res.n_barcodes == 40
    c.close()


# ------------------------------------------------------------------ 7. errors
def test_errors_and_a_refused_call_adds_nothing():
    w = _world("syn")
    b, r = _syn_run()
    a = w.aligner(capi.CI_OPTS)
    for args in ((2, 16, 12), (0, 0, 12), (0, 17, 12), (0, 16, 0), (0, 16, 17)):
        e = _raises(lambda: capi.Cells(a, *args))
        assert e.code == capi.ERR_INVALID_ARG, args
    c = capi.Cells(a)
    # a batch that went up without names: the BAM layer's message
    small = _part(b, 0, 300)
    a.upload(small["bases"], small["offsets"])
    a.run()
    e_bam, e = _raises(a.fetch_bam), _raises(c.add)
    assert (e.code, str(e)) == (e_bam.code, str(e_bam)) and e.code == capi.ERR_INVALID_ARG and "names" in str(e)
    assert _raises(lambda: c.fetch(0)).code == capi.ERR_INVALID_ARG
    # add_view: name offsets that do not start at 0, or descend
    offsets, alns, dig, words = qc.uniform_view(4, 1, 0, 1000, 0, [(91, "M")])
    pool, name_off = cl.join_names([b"a_" + b"A" * 16 + b"_" + b"C" * 12] * 4)
    c.add_view(offsets, alns, dig, words, pool, name_off)
    before = _bytes_of(c.fetch())
    bad = name_off.copy()
    bad[2] = bad[1] - 1
    e = _raises(lambda: c.add_view(offsets, alns, dig, words, pool, bad))
    assert e.code == capi.ERR_INVALID_ARG and "read 1" in str(e)
    bad = name_off.copy()
    bad[0] = 1
    assert _raises(lambda: c.add_view(offsets, alns, dig, words, pool, bad)).code == capi.ERR_INVALID_ARG
    bad_alns = alns.copy()
    bad_alns["tx_or_gene_idx"][3] = len(w.t["txs"])
    assert "alignment 3" in str(_raises(lambda: c.add_view(offsets, bad_alns, dig, words, pool, name_off)))
    assert _bytes_of(c.fetch()) == before
    c.close()
    # a cap that the first add fits and the second does not
    first, second = _part(b, 0, 1500), _part(b, 1500, 4000)
    probe = capi.Cells(a)
    n1 = _add_reads(a, probe, first)["n_molecules"]
    probe.close()
    capped = capi.Cells(a, 0, 16, 12, 16 * n1)
    assert _add_reads(a, capped, first)["n_molecules"] == n1
    before = _bytes_of(capped.fetch())
    a.upload_reads(second)
    a.run()
    e = _raises(capped.add)
    assert e.code == capi.ERR_OOM and str(16 * n1) in str(e) and "bytes" in str(e)
    assert _bytes_of(capped.fetch()) == before
    # ... the same reads again bring no new molecule, and fit
    _add_reads(a, capped, first)
    assert capped.fetch().n_molecules == n1
    capped.close()
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
    e = _raises(lambda: capi.Cells(a))
    assert (e.code, str(e)) == (e_bam.code, str(e_bam)) and e.code == capi.ERR_INVALID_ARG and "names" in str(e)
    a.close()
    ix.close()


# ------------------------------------------------------------------ 8. nothing is disturbed
@pytest.mark.parametrize("cells_first", [True, False], ids=["cells_first", "quant_first"])
def test_add_disturbs_no_view_counter_or_timing(cells_first):
    w = _world("syn")
    b, r = _syn_run()
    part = _part(b, 0, 500)
    a = w.aligner(capi.CI_OPTS)

    def run(with_cells):
        """fetch, fetch_cigars, fetch_bam, a Quant.add and (with_cells) a Cells.add on one run -> everything they returned"""
        a.upload_reads(part)
        a.run()
        q, c = capi.Quant(a), capi.Cells(a) if with_cells else None
        got = {}
        steps = ["cells", "quant"] if cells_first else ["quant", "cells"]
        views = (a.fetch(), a.fetch_cigars(), a.fetch_bam())
        counters, timings = a.counters().copy(), a.timings()
        for s in steps:
            if s == "quant":
                info = q.add()
                got["quant"] = {k: v for k, v in info.items() if k not in ("add_ms", "held_bytes")}
            elif with_cells:
                info = c.add()
                assert info["n_reads"] == 500 and info["add_ms"] > 0
            assert np.array_equal(a.counters(), counters) and a.timings() == timings, s
        got["counters"] = counters
        again = (a.fetch(), a.fetch_cigars(), a.fetch_bam())
        fields = [("offsets", "alns", "ops"), ("offsets", "alns", "digests", "cigar"), ("data", "read_rec_off")]
        for v, v2, fs in zip(views, again, fields):
            for f in fs:
                assert np.array_equal(getattr(v, f), getattr(v2, f)), f
        got["views"] = [[getattr(v, f) for f in fs] for v, fs in zip(again, fields)]
        got["quant_tables"] = qc.pack(qc.of_result(q.fetch()))
        if with_cells:
            a0 = int(r.offsets[500])
            mol, tot = cl.expected(w.t, r.offsets[:501], r.alns[:a0], None, part["names"], part["name_off"], 0, 16, 12)
            cl.assert_result(c.fetch(), mol, tot)
            c.close()
        q.close()
        return got

    a.reset_counters()
    plain = run(False)
    a.reset_counters()
    with_cells = run(True)
    assert np.array_equal(plain["counters"], with_cells["counters"])
    assert plain["quant"] == with_cells["quant"] and plain["quant_tables"] == with_cells["quant_tables"]
    for x, y in zip(plain["views"], with_cells["views"]):
        for u, v in zip(x, y):
            assert np.array_equal(u, v)
    a.close()
