"""Reference and reads of tests/test_gpu_seed_direct.py, shared with tests/seed_direct_child.py: parent and child build
identical inputs from fixed seeds.

One text of two contigs (45 and 6 kilobases, an N run, exact 12-mers planted 2 to 70 times), indexed with THM_KT = 8, so
that the k-mer table has buckets of every size the seed probe tells apart: empty, one suffix (the entries whose device
copy holds the text position, thermite_amd/csrc/lut_direct.h), 2..8 (all suffixes fetched together), 9 and more (binary
search).  The reads are cut from the text at positions chosen by looking the bucket sizes up in the host's table, and
each case puts its k-mer at read position 0, which is always probed in full."""
import os

import numpy as np

from thermite_amd import capi, refdata, synth

KT = 8
K = 20
L = 91
ACGT = np.frombuffer(b"ACGT", np.uint8)
MAIN_LEN, SECOND_LEN = 45000, 6000
N_RUN = (15000, 15200)
PLANT = [(2, 6), (3, 3), (7, 6), (8, 8), (9, 8), (10, 4), (64, 2), (70, 1)]   # (copies, different 12-mers planted that often)
TAIL_SUBS = (0, 1, 7, 8, 55, 56, 63, 64, 65, 71, 72, 73, 79, 80, 81)          # tail bytes (behind the kt-mer) that get a substitution

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def other(*avoid):
    return int([b for b in ACGT if int(b) not in [int(a) for a in avoid]][0])


def sub(read, p):
    r = np.array(read, np.uint8)
    r[p] = other(r[p])
    return r


def _make_tables():
    rng = np.random.Generator(np.random.PCG64(0xD12EC7))
    main = ACGT[rng.integers(0, 4, MAIN_LEN)].copy()
    main[N_RUN[0]: N_RUN[1]] = ord("N")
    at = 20000   # the planted copies stand behind the genes and the N run, 40..70 (the two biggest families 14..30) bases apart
    for copies, kinds in PLANT:
        for _ in range(kinds):
            m = ACGT[rng.integers(0, 4, 12)]
            for _ in range(copies):
                main[at: at + 12] = m
                at += int(rng.integers(40, 70)) if copies < 60 else int(rng.integers(14, 30))
    assert at < MAIN_LEN - 2000, at
    second = ACGT[rng.integers(0, 4, SECOND_LEN)].copy()
    genes, txs = synth.synth_annotation(rng, "main", 14000, 100, 4)
    return refdata.build_tables([("main", main), ("second", second)], genes, txs)


def tables():
    return _once("tables", _make_tables)


def make_index(t, wide):
    """an index with THM_KT = 8 (read when the index is created)"""
    old = os.environ.get("THM_KT")
    os.environ["THM_KT"] = str(KT)
    try:
        return capi.Index(t, wide=wide)
    finally:
        if old is None:
            del os.environ["THM_KT"]
        else:
            os.environ["THM_KT"] = old


def host_view():
    """(text, suffix array, host k-mer table as int64, bucket size of the kt-mer at every text position or -1)"""
    def make():
        t = tables()
        ix = make_index(t, False)
        sa = ix.suffix_array().astype(np.int64)
        lut = ix.debug_host_lut().astype(np.int64)
        ix.close()
        assert lut.shape[0] == 4 ** KT
        text = t["text"]
        code_of = np.full(256, -1, np.int64)
        code_of[ACGT] = np.arange(4)
        c = code_of[text]
        n = len(text)
        code = np.zeros(n, np.int64)
        ok = np.ones(n, bool)
        for j in range(KT):
            cj = np.full(n, -1, np.int64)
            cj[: n - j] = c[j:]
            ok &= cj >= 0
            code = code * 4 + np.maximum(cj, 0)
        size = np.where(ok, lut[code, 1] - lut[code, 0], -1)
        return text, sa, lut, size
    return _once("host_view", make)


def _window_ok(text, p, n):
    return p >= 0 and p + n <= len(text) and not np.isin(text[p: p + n], [ord("$"), ord("N")]).any()


def positions_with_bucket(pred, n_want, need=L, skip=0):
    """text positions, spread over the text, whose kt-mer sits in a bucket of a size `pred` accepts and that have
    `need` bases without '$' or N behind them"""
    text, _, _, size = host_view()
    cand = np.nonzero(pred(size))[0]
    out = []
    step = max(1, len(cand) // (4 * n_want + 1))
    for p in cand[skip::step]:
        if _window_ok(text, int(p), need):
            out.append(int(p))
            if len(out) == n_want:
                break
    assert len(out) == n_want, (len(out), n_want)
    return out


def _absent_kmer():
    _, _, lut, _ = host_view()
    empty = np.nonzero(lut[:, 1] == lut[:, 0])[0]
    assert len(empty) > 100
    out = []
    for code in empty[:: len(empty) // 6][:6]:
        out.append(np.array([ACGT[(int(code) >> (2 * (KT - 1 - j))) & 3] for j in range(KT)], np.uint8))
    return out


def _make_cases():
    """name -> list of reads"""
    text, sa, lut, size = host_view()
    t = tables()
    rng = np.random.Generator(np.random.PCG64(0x5EED1D))
    one = lambda s: s == 1   # noqa: E731
    cases = {}
    p1 = positions_with_bucket(one, 6)
    # the whole read matches, its kt-mer at position 0 in a one-suffix bucket; both strands of the text and of the read
    cases["one_exact"] = [text[p: p + L].copy() for p in p1] + [refdata.revcomp(text[p: p + L]) for p in p1[:3]]
    cases["one_exact"] += [text[p: p + n].copy() for p in p1[:2] for n in (88, 89, 90)]    # tails of 80, 81, 82 bytes
    # a substitution on tail byte j (j = 0: right behind the kt-mer, the compare returns 0; 63 | 64: the boundary of a
    # round trip of eight text words; 79 | 80: that of the ten-word compare DESIGN.md section 4.1 measured and dropped),
    # at read lengths whose tails end at and behind 80 bytes
    cases["one_tail_sub"] = [sub(text[p: p + n], KT + j) for p in p1[:2] for n in (88, 89, L) for j in TAIL_SUBS if KT + j < n]
    cases["one_tail_sub"] += [sub(text[p: p + n], n - 1) for p in p1[:2] for n in (88, 89, L)]
    # one substitution anywhere: the probes behind position 0 (grid and fill), with and without a hint
    cases["one_sub_anywhere"] = [sub(text[p: p + L], q) for p in p1[2:4] for q in range(0, L, 2)]
    # buckets of 2, 8, 9 and >= 60 suffixes: a read from every (up to 4) occurrence, exact and with a substitution
    for name, pred in (("bucket_2", lambda s: s == 2), ("bucket_8", lambda s: s == 8), ("bucket_9", lambda s: s == 9),
                       ("bucket_60", lambda s: s >= 60)):
        reads = []
        for p in positions_with_bucket(pred, 3):
            code = 0
            for b in text[p: p + KT]:
                code = code * 4 + int(np.nonzero(ACGT == b)[0][0])
            occ = [int(x) for x in sa[lut[code, 0]: lut[code, 1]]]
            assert p in occ
            for o in ([p] + [x for x in occ if x != p])[:4]:
                if _window_ok(text, o, L):
                    reads += [text[o: o + L].copy(), sub(text[o: o + L], 30), sub(text[o: o + L], KT), sub(text[o: o + L], 12)]
        assert len(reads) >= 12, name
        cases[name] = reads
    # kt-mer absent from the text, in front of random bases and in front of text
    cases["absent"] = [np.concatenate([m, ACGT[rng.integers(0, 4, L - KT)]]) for m in _absent_kmer()]
    cases["absent"] += [np.concatenate([m, text[p1[0]: p1[0] + L - KT]]) for m in _absent_kmer()[:2]]
    # N (and bytes outside ACGTN) inside the kt-mer and right behind it
    reads = []
    for p in p1[:2]:
        for at in (0, 3, KT - 1, KT, KT + 1):
            for c in (b"N", b"n", b"*"):
                r = text[p: p + L].copy()
                r[at] = c[0]
                reads.append(r)
    cases["n_in_read"] = reads
    # a one-suffix bucket whose suffix lies within L of a contig end: the compare runs into '$' (both contigs, both strands)
    reads = []
    for r in t["refs"]:
        end = int(r["end_idx"]) - 1            # the '$'
        for back in (KT, KT + 1, 20, 30, 47, 64, 72, 79, 80, 81):
            p = end - back
            while size[p] != 1:
                p -= 1
            back = end - p
            assert back <= L
            reads.append(np.concatenate([text[p: end], ACGT[rng.integers(0, 4, L - back)]]))
            reads.append(text[p: end].copy())                  # the read ends where the contig does
    # ... and within L of the N run
    for back in (KT, 20, 64, 65, 80):
        p = N_RUN[0] - back
        while size[p] != 1:
            p -= 1
        reads.append(np.concatenate([text[p: N_RUN[0]], ACGT[rng.integers(0, 4, L - (N_RUN[0] - p))]]))
        reads.append(text[p: p + L].copy())                    # N against N matches
    cases["contig_end"] = reads
    # reads of k - 1, k and k + 1 bases
    cases["short"] = [text[p: p + n].copy() for p in p1[:3] for n in (K - 1, K, K + 1)] + \
                     [sub(text[p: p + n], n - 1) for p in p1[:3] for n in (K, K + 1)]
    return cases


def cases():
    return _once("cases", _make_cases)


def case_batch(name):
    """(bases, offsets) of a case; name 'all': every case in one batch"""
    def make():
        c = cases()
        reads = c[name] if name != "all" else [r for n in sorted(c) for r in c[n]]
        return refdata.pack_reads([np.asarray(r, np.uint8) for r in reads])
    return _once(("batch", name), make)


OPTS = dict(capi.CI_OPTS, min_seed_len=K)


def device_run(ix, bases, off, seed_direct=None):
    """what the child saves and the parent compares: thm_smems_batch and thm_align_batch of one batch with the seed
    probes counted, the device table and the counts"""
    out = {}
    a = capi.Aligner(ix, dict(capi.DEFAULT_OPTS, min_seed_len=K))
    a.debug_set_flags(seed_stats=True, seed_direct=seed_direct)
    out["lut"] = a.debug_fetch_lut(ix.debug_host_lut())
    out["smem_off"], out["smem_mems"] = a.smems_batch(bases, off, K)
    out["smem_direct"] = np.array(a.debug_seed_direct_stats(), "<u8")
    out["smem_stats"] = np.array(a.debug_seed_stats(), "<u8")
    a.close()
    a = capi.Aligner(ix, OPTS)
    a.debug_set_flags(seed_stats=True, seed_direct=seed_direct)
    a.reset_counters()
    g = a.align_batch(bases, off)
    assert g.n_failed == 0 and g.status is None
    out["offsets"], out["alns"], out["ops"] = g.offsets, g.alns, g.ops
    out["counters"] = np.array(a.counters(), "<u8")
    out["direct"] = np.array(a.debug_seed_direct_stats(), "<u8")
    out["stats"] = np.array(a.debug_seed_stats(), "<u8")
    a.close()
    return out
