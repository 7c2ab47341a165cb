"""-m gpu: the per-hit entry points -- thm_extend_left_right_batch (extend_left_right, reference src/aligner.rs:352-407)
and thm_align_seed_hits_batch (align_seed_hit, src/aligner.rs:198-314) -- against the CPU oracle.  The oracle has no
align_seed_hit entry of its own, so `expected_hit` below restates src/aligner.rs:198-314,429-449 from the primitives it
binds (Swg.extend_left_right, extend_seed_match, lift_mem_to_tx, lift_tx_to_gx, the two interval trees)."""
import json
import os

import numpy as np
import pytest

from oracle import pyoracle as orc
from thermite_amd import capi, refdata, synth

from gpu_common import World, _tx_exons, assert_hits_equal, check_align, expected_batch, expected_hit, initial_band, mutate

pytestmark = pytest.mark.gpu

_ACGT = np.frombuffer(b"ACGT", np.uint8)


_worlds = {}


def _world(key, make, wide):
    if (key, wide) not in _worlds:
        _worlds[(key, wide)] = World(make(), wide)
    return _worlds[(key, wide)]


@pytest.fixture(params=[False, True], ids=["c32", "c64"])
def test_ref(request, data_dir):
    return _world("test_ref", lambda: refdata.load_reference(data_dir + "/test_ref.fasta", data_dir + "/test_ref.gtf"), request.param)


@pytest.fixture(params=[False, True], ids=["c32", "c64"])
def chrm(request, data_dir):
    return _world("chrm", lambda: refdata.load_reference(data_dir + "/GRCh38-2020-A-chrM.fasta", data_dir + "/GRCh38-2020-A-chrM.gtf"),
                  request.param)


@pytest.fixture(params=[False, True], ids=["c32", "c64"])
def syn(request):
    return _world("syn", lambda: synth.synth_reference(length=400000, n_genes=40), request.param)


@pytest.fixture(scope="module")
def chrm32(data_dir):
    return _world("chrm", lambda: refdata.load_reference(data_dir + "/GRCh38-2020-A-chrM.fasta", data_dir + "/GRCh38-2020-A-chrM.gtf"),
                  False)


def _mutated_reads(rng, t, n, L):
    bases, off, _ = synth.simulate_reads(t, n, L, sub_rate=0.03, indel_rate=0.006, intronic_frac=0.25, stream=int(rng.integers(1000)))
    return bases, off


def _hits_for(w, bases, off, rng, narrow, k=None):
    hit_off, hits = w.a.smems_batch(bases, off, k or capi.CI_OPTS["min_seed_len"])
    lens = np.diff(off.astype(np.int64))
    per_hit_len = np.repeat(lens, np.diff(hit_off.astype(np.int64)))
    bw0 = np.array([initial_band(capi.CI_OPTS, int(L)) for L in per_hit_len], "<u4")
    if narrow:
        bw = (bw0 * rng.random(len(bw0))).astype("<u4")
        xd = (bw + rng.integers(0, 6, len(bw))).astype("<i4")
    else:
        bw, xd = bw0, bw0.astype("<i4")
    return hit_off, hits, bw, xd, int(bw0.max(initial=0))


# ------------------------------------------------------------------ tests
def test_extend_left_right_reference_vector(chrm32, golden_dir):
    """src/aligner.rs:603-639 test_extend_left_right through the HIP kernel: every field and op byte"""
    kat = json.load(open(os.path.join(golden_dir, "reference_kats.json")))["extend_left_right"]
    read, ref = kat["read"].encode(), kat["ref"].encode()
    hit = np.zeros(1, capi.MEM_DT)
    hit[0] = (kat["hit"]["ref_idx"], kat["hit"]["query_idx"], kat["hit"]["len"])
    alns, ops = chrm32.a.extend_left_right_batch(read, [0, len(read)], ref, [0, len(ref)], hit, [kat["bw"]], [kat["xd"]],
                                                 kat["max_band_width"])
    a = alns[0]
    for f in ("score", "ystart", "xstart", "yend", "xend", "ylen", "xlen"):
        assert int(a[f]) == kat[f], f
    exp_ops = [tuple(o) if isinstance(o, list) else o for o in kat["ops"]]
    assert orc.decode_ops(ops[a["ops_off"]: a["ops_off"] + a["ops_len"]]) == exp_ops
    assert a["ops_off"] == 0 and a["ops_len"] == len(ops)


def _elr_problems(rng, n):
    xs, ys, hits, bws, xds = [], [], [], [], []
    for i in range(n):
        L = int(rng.integers(0, 320))
        read = _ACGT[rng.integers(0, 4, L)]
        ln = int(rng.integers(0, L + 1)) if L else 0
        q = int(rng.integers(0, L - ln + 1))
        kind = i % 4
        if kind == 0:
            q = 0  # empty left side
        elif kind == 1:
            q = L - ln  # empty right side
        flank_l, flank_r = int(rng.integers(0, 400)), int(rng.integers(0, 400))
        if kind == 2:
            flank_l, flank_r = int(rng.integers(0, 4)), int(rng.integers(0, 4))  # near the reference ends
        body = mutate(rng, read, sub=rng.random() * 0.1, indel=rng.random() * 0.04)
        ref = np.concatenate([_ACGT[rng.integers(0, 4, flank_l)], body, _ACGT[rng.integers(0, 4, flank_r)]]).astype(np.uint8)
        ln = min(ln, len(ref))
        r = max(0, min(flank_l + q, len(ref) - ln))  # not necessarily an exact match
        bw = int(rng.choice([0, 1, 3, 10, 30, 63, 64, 100, 127, 128, 150, 200]))
        xs.append(read)
        ys.append(ref)
        hits.append((r, q, ln))
        bws.append(bw)
        xds.append(bw + int(rng.integers(0, 5)))
    xb, xo = refdata.pack_reads(xs)
    yb, yo = refdata.pack_reads(ys)
    h = np.zeros(n, capi.MEM_DT)
    for i, v in enumerate(hits):
        h[i] = v
    return xb, xo, yb, yo, h, np.array(bws, "<u4"), np.array(xds, "<i4")


def test_extend_left_right_fuzz(chrm32):
    rng = np.random.default_rng(11)
    xb, xo, yb, yo, hits, bw, xd = _elr_problems(rng, 3000)
    max_bw = int(bw.max())
    # one call per band class as well as one call over all of them (the any-width kernel takes the wide bands)
    for sel in (bw <= 31, (bw > 31) & (bw <= 127), np.ones(len(bw), bool)):
        idx = np.nonzero(sel)[0]
        xs = [xb[xo[i]: xo[i + 1]] for i in idx]
        ys = [yb[yo[i]: yo[i + 1]] for i in idx]
        sxb, sxo = refdata.pack_reads(xs)
        syb, syo = refdata.pack_reads(ys)
        alns, ops = chrm32.a.extend_left_right_batch(sxb, sxo, syb, syo, hits[idx], bw[idx], xd[idx], max_bw)
        swg = orc.Swg(max_bw)
        for j, i in enumerate(idx):
            e = swg.extend_left_right(ys[j], tuple(int(v) for v in hits[i]), xs[j], int(bw[i]), int(xd[i]))
            a = alns[j]
            got = (int(a["score"]), int(a["ystart"]), int(a["xstart"]), int(a["yend"]), int(a["xend"]), int(a["ylen"]), int(a["xlen"]))
            assert got == (e["score"], e["ystart"], e["xstart"], e["yend"], e["xend"], e["ylen"], e["xlen"]), (i, got, e)
            assert orc.decode_ops(ops[a["ops_off"]: a["ops_off"] + a["ops_len"]]) == e["ops"], i
        assert int(alns["ops_len"].astype(np.int64).sum()) == len(ops)


def test_extend_left_right_out_of_contract(chrm32):
    read, ref = b"ACGTACGT", b"ACGTACGTAA"
    for hit, bw, xd in (((0, 6, 3), 1, 1), ((9, 0, 2), 1, 1), ((0, 0, 4), 5, 5), ((0, 0, 4), 2, 1)):
        h = np.zeros(1, capi.MEM_DT)
        h[0] = hit
        with pytest.raises(capi.ThermiteError) as e:
            chrm32.a.extend_left_right_batch(read, [0, 8], ref, [0, 10], h, [bw], [xd], 4)
        assert e.value.code == capi.ERR_OUT_OF_CONTRACT


def _check_world(w, n_reads, L, seed, reads=None, k=None):
    rng = np.random.default_rng(seed)
    bases, off = reads if reads is not None else _mutated_reads(rng, w.t, n_reads, L)
    for narrow in (False, True):
        hit_off, hits, bw, xd, max_bw = _hits_for(w, bases, off, rng, narrow, k)
        assert len(hits) > 0
        before = w.a.counters()
        got = w.a.align_seed_hits(bases, off, hit_off, hits, bw, xd, max_bw)
        after = w.a.counters()
        assert_hits_equal(got, expected_batch(w, bases, off, hit_off, hits, bw, xd, max_bw), "narrow" if narrow else "initial")
        d = after.astype(np.int64) - before.astype(np.int64)
        assert d[capi.COUNTER_NAMES.index("hits")] == len(hits)
        assert d[capi.COUNTER_NAMES.index("op_bytes")] == len(got[1])
        assert d[capi.COUNTER_NAMES.index("reads")] == 0 and d[capi.COUNTER_NAMES.index("alns")] == 0


def test_align_seed_hits_test_ref(test_ref, data_dir):
    """the reference's own test query (BASELINE config 1: -k3), mutated copies of it"""
    rng = np.random.default_rng(1)
    _, seqs, _ = refdata.parse_fastq(data_dir + "/test_query.fastq")
    seqs = [np.frombuffer(bytes(s), np.uint8) for s in seqs]
    seqs = seqs + [mutate(rng, s) for s in seqs for _ in range(3)]
    _check_world(test_ref, 0, 0, 1, reads=refdata.pack_reads(seqs), k=3)


def test_align_seed_hits_chrm(chrm):
    _check_world(chrm, 300, 91, 2)


def test_align_seed_hits_synthetic(syn):
    """multi-exon transcripts on both strands, 150-base reads (bands of three cells per lane)"""
    _check_world(syn, 200, 91, 3)
    _check_world(syn, 60, 150, 4)


def _short_intron_reference(seed=0x696E7472):
    """One random contig whose transcripts have two or three exons of 36..44 bases separated by introns of 6..10 bases
    (shorter than min_seed_len = 20), on both strands; every three-exon gene has a second isoform without the middle
    exon.  tables["_spans"]: each gene's (first exon start, last exon end) on the contig."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_genes, slot = 60, 400
    name = "shortintron"
    seq = _ACGT[rng.integers(0, 4, n_genes * slot + 200)]
    genes, txs, spans = [], [], []
    for g in range(n_genes):
        n_ex = 2 + g % 2
        p = 100 + g * slot + int(rng.integers(0, 100))
        exons = []
        for _ in range(n_ex):
            e = p + int(rng.integers(36, 45))
            exons.append((p, e))
            p = e + int(rng.integers(6, 11))
        strand = bool(g % 4 < 2)
        genes.append(dict(id="SIG%03d" % g, name="si%d" % g))
        txs.append(dict(id="SIT%03d.0" % g, gene_idx=g, chrom=name, strand=strand, exons=exons))
        if n_ex == 3:
            txs.append(dict(id="SIT%03d.1" % g, gene_idx=g, chrom=name, strand=strand, exons=[exons[0], exons[2]]))
        spans.append((exons[0][0], exons[-1][1]))
    t = refdata.build_tables([(name, seq)], genes, txs)
    t["_spans"] = spans
    return t


@pytest.fixture(params=[False, True], ids=["c32", "c64"])
def short_introns(request):
    return _world("short_introns", _short_intron_reference, request.param)


def _seeds_meeting_two_exons(t, hits):
    """hits whose seed [ref_idx, ref_idx + len) intersects at least two exons of one transcript"""
    s = hits["ref_idx"].astype(np.int64)
    e = s + hits["len"].astype(np.int64)
    found = np.zeros(len(hits), bool)
    for tx_idx in range(len(t["txs"])):
        met = np.zeros(len(hits), np.int64)
        for x0, x1, _ in _tx_exons(t, tx_idx):
            met += (s < x1) & (x0 < e)
        found |= met >= 2
    return int(found.sum())


def test_seed_across_short_intron(short_introns):
    """Reads copied from the genome across introns shorter than min_seed_len: their seeds run through an intron into the
    transcript's next exon, so the exon grid yields an entry whose previous exon reaches into the seed, and
    lift_mem_to_tx (src/txome.rs:82-103) takes its general case, the first exon in transcript order that intersects
    the seed (extend_device.h, lift_seed_to_tx).  Read level (thm_align_batch) and hit level (thm_align_seed_hits_batch)."""
    w = short_introns
    rng = np.random.default_rng(9)
    fwd = w.t["text"][: int(w.t["refs"][0]["len"])]
    reads = []
    for i in range(240):
        lo, hi = w.t["_spans"][i % len(w.t["_spans"])]
        s = int(rng.integers(lo - 20, hi - 91 + 20))  # every 91-base window here holds an intron and part of both exons beside it
        r = mutate(rng, fwd[s: s + 91], sub=0.015, indel=0.0)
        reads.append(refdata.revcomp(r) if i % 3 == 2 else r)
    bases, off = refdata.pack_reads(reads)
    _, hits = w.a.smems_batch(bases, off, capi.CI_OPTS["min_seed_len"])
    assert _seeds_meeting_two_exons(w.t, hits) > 0
    check_align(w, bases, off, capi.CI_OPTS)
    _check_world(w, 0, 0, 9, reads=(bases, off))


def test_consistent_with_align_batch(syn):
    """a read whose SMEMs give one hit, and whose alignment passes align_read's filters, gets the per-hit record from
    thm_align_batch (with primary = 1)"""
    rng = np.random.default_rng(5)
    opts = capi.CI_OPTS
    bases, off = _mutated_reads(rng, syn.t, 2000, 91)
    hit_off, hits = syn.a.smems_batch(bases, off, opts["min_seed_len"])
    one = np.nonzero(np.diff(hit_off.astype(np.int64)) == 1)[0]
    assert len(one) > 100
    bw0 = initial_band(opts, 91)
    hits1 = hits[hit_off[one]]
    sel_b = np.concatenate([bases[off[r]: off[r + 1]] for r in one])
    sel_o = np.concatenate([[0], np.cumsum(np.diff(off.astype(np.int64))[one])]).astype("<u8")
    n = len(one)
    alns, ops, st = syn.a.align_seed_hits(sel_b, sel_o, np.arange(n + 1, dtype="<u8"), hits1, np.full(n, bw0, "<u4"),
                                          np.full(n, bw0, "<i4"), bw0)
    assert not st.any()
    res = syn.a.align_batch(sel_b, sel_o)
    compared = 0
    for i in range(n):
        if res.offsets[i + 1] - res.offsets[i] != 1:
            continue
        ref = res.alns[res.offsets[i]].copy()
        mine = alns[i].copy()
        assert mine["primary"] == 0
        mine["primary"] = 1
        for f in ("ops_off", "tx_ops_off"):
            mine[f] = ref[f] = 0
        assert mine == ref, (i, mine, ref)
        a0, t0 = int(alns[i]["ops_off"]), int(res.alns[res.offsets[i]]["ops_off"])
        nb = int(ref["ops_len"]) + int(ref["tx_ops_len"])
        assert np.array_equal(ops[a0: a0 + nb], res.ops[t0: t0 + nb]), i
        compared += 1
    assert compared > 100


def test_per_hit_statuses(chrm32):
    w = chrm32
    rng = np.random.default_rng(6)
    bases, off = _mutated_reads(rng, w.t, 40, 91)
    hit_off, hits, bw, xd, max_bw = _hits_for(w, bases, off, rng, False)
    hits, bw, xd = hits.copy(), bw.copy(), xd.copy()
    n_text = len(w.t["text"])
    refs = w.t["refs"]
    bad = {}
    nz = np.nonzero(np.diff(hit_off.astype(np.int64)) >= 1)[0]
    picks = [int(hit_off[r]) for r in nz[:8]]
    # beyond the text; crossing the end of its contig copy; band wider than max_band_width; x_drop < band_width;
    # query_idx + len beyond the read
    hits[picks[0]]["ref_idx"] = n_text + 5
    e0 = int(refs[0]["end_idx"])
    hits[picks[1]]["ref_idx"] = e0 - 1 - int(hits[picks[1]]["len"]) + 3
    bw[picks[2]] = max_bw + 1
    xd[picks[3]] = int(bw[picks[3]]) - 1
    hits[picks[4]]["query_idx"] = 91 - int(hits[picks[4]]["len"]) + 1
    for p in picks[:5]:
        bad[p] = capi.ERR_OUT_OF_CONTRACT
    alns, ops, st = w.a.align_seed_hits(bases, off, hit_off, hits, bw, xd, max_bw)
    for p, code in bad.items():
        assert st[p] == code, (p, st[p])
        assert alns[p]["ops_len"] == 0 and alns[p]["score"] == 0
    good = np.ones(len(hits), bool)
    good[list(bad)] = False
    assert not st[good].any()
    # the neighbours equal the restatement
    keep_r = [r for r in range(len(off) - 1) if all(not (hit_off[r] <= p < hit_off[r + 1]) for p in bad)]
    for r in keep_r[:10]:
        h0, h1 = int(hit_off[r]), int(hit_off[r + 1])
        swg = orc.Swg(max_bw)
        read = bytes(bases[off[r]: off[r + 1]])
        for h in range(h0, h1):
            rec, b = expected_hit(w, swg, read, (int(hits[h]["ref_idx"]), int(hits[h]["query_idx"]), int(hits[h]["len"])), int(bw[h]), int(xd[h]))
            got = alns[h].copy()
            a0 = int(got["ops_off"])
            assert bytes(ops[a0: a0 + len(b)]) == b
            rec["ops_off"], got["ops_off"], rec["tx_ops_off"], got["tx_ops_off"] = 0, 0, 0, 0
            assert got == rec, h


def test_empty_and_sparse_calls(chrm32):
    w = chrm32
    rng = np.random.default_rng(7)
    bases, off = _mutated_reads(rng, w.t, 30, 91)
    # n_hits = 0
    alns, ops, st = w.a.align_seed_hits(bases, off, np.zeros(len(off), "<u8"), np.zeros(0, capi.MEM_DT), [], [], 10)
    assert len(alns) == 0 and len(ops) == 0 and len(st) == 0
    # reads without hits between reads with hits
    hit_off, hits, bw, xd, max_bw = _hits_for(w, bases, off, rng, False)
    keep = np.ones(len(hits), bool)
    for r in range(1, len(off) - 1, 2):
        keep[int(hit_off[r]): int(hit_off[r + 1])] = False
    counts = np.diff(hit_off.astype(np.int64))
    counts[1::2] = 0
    ho = np.concatenate([[0], np.cumsum(counts)]).astype("<u8")
    got = w.a.align_seed_hits(bases, off, ho, hits[keep], bw[keep], xd[keep], max_bw)
    assert_hits_equal(got, expected_batch(w, bases, off, ho, hits[keep], bw[keep], xd[keep], max_bw), "sparse")
    # hit_off[n_reads] != n_hits: the whole call fails
    with pytest.raises(capi.ThermiteError) as e:
        w.a.align_seed_hits(bases, off, ho + 1, hits[keep], bw[keep], xd[keep], max_bw)
    assert e.value.code == capi.ERR_INVALID_ARG


def test_long_read_wide_band(chrm32):
    """a 300-base read at band 200: the any-width kernel"""
    w = chrm32
    rng = np.random.default_rng(8)
    bases, off, _ = synth.simulate_reads(w.t, 30, 300, sub_rate=0.03, indel_rate=0.006, stream=88)
    hit_off, hits = w.a.smems_batch(bases, off, 20)
    n = len(hits)
    bw = np.full(n, 200, "<u4")
    xd = np.full(n, 200, "<i4")
    got = w.a.align_seed_hits(bases, off, hit_off, hits, bw, xd, 200)
    assert_hits_equal(got, expected_batch(w, bases, off, hit_off, hits, bw, xd, 200), "bw200")
