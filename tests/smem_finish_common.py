"""Shared by tests/test_smem_finish_host.py and tests/test_gpu_smem_finish.py: the references and read batches of the
finisher's cases (thermite_amd/csrc/smem_finish.h: class E, whole-read exact matches; class S, one substitution between
two SMEMs), the stand-alone host program over the header (tests/cpp/smem_finish_main.cpp) and its comparison with the CPU
oracle.  Everything comes from seeded generators."""
import os
import struct
import subprocess

import numpy as np

from thermite_amd import capi, refdata, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ACGT = np.frombuffer(b"ACGT", np.uint8)
L0 = 91
CLASS_E, CLASS_S = 1, 2
OUT_DT = np.dtype([(f, "<i8") for f in (
    "what", "shape", "accepted", "ystart", "yend", "ylen", "tx_ystart", "tx_yend", "tx_ylen", "ops_off", "tx_ops_off", "score",
    "ref_id", "name_rank", "type_idx", "strand", "aln_type", "calls", "window_bytes", "op_bytes")])
EXONIC = 0


# ------------------------------------------------------------------ references
def planted_reference(seed=0x66696E):
    """A random 120 kb contig with what the two generated references do not have: an exon that a shorter exon of another
    isoform overlaps, a run of 21 equal bases and a two-letter repeat inside an exon, a '-' strand gene, and a 150-mer that
    occurs twice.  Returns (tables, info)."""
    rng = np.random.Generator(np.random.PCG64([seed, 1]))
    seq = _ACGT[rng.integers(0, 4, 120000)].copy()
    seq[10199] = ord("C")
    seq[10200:10221] = ord("A")
    seq[10221] = ord("G")
    seq[10300:10330] = np.frombuffer(b"AC" * 15, np.uint8)
    seq[50000:50150] = seq[40000:40150]
    genes = [dict(id="G%d" % k, name="g%d" % k) for k in range(4)]
    txs = [
        dict(id="T0", gene_idx=0, chrom="planted", strand=True, exons=[(5000, 5400), (6000, 6300)]),
        dict(id="T1", gene_idx=0, chrom="planted", strand=True, exons=[(5100, 5200), (6000, 6300)]),
        dict(id="T2", gene_idx=1, chrom="planted", strand=True, exons=[(10000, 10500)]),
        dict(id="T3", gene_idx=2, chrom="planted", strand=False, exons=[(20000, 20400), (21000, 21400)]),
        dict(id="T4", gene_idx=3, chrom="planted", strand=True, exons=[(39900, 40300)]),
    ]
    t = refdata.build_tables([("planted", seq)], genes, txs)
    return t, dict(overlap=(5000, 5400, 5100, 5200), homopolymer=(10200, 10221), dinuc=(10300, 10330), repeat=(40000, 50000, 150),
                   minus=(20000, 20400), exon=(10000, 10500))


def forward(t):
    return t["text"][: int(t["refs"][0]["len"])]


def exons_forward(t):
    """(start, end) of every exon on the forward copy of the first contig, in contig coordinates, distinct"""
    r0 = t["refs"][0]
    e = t["exons"]
    on = (e["start"] >= r0["start_idx"]) & (e["end"] <= r0["end_idx"])
    s = np.unique(np.stack([e["start"][on] - r0["start_idx"], e["end"][on] - r0["start_idx"]], axis=1).astype(np.int64), axis=0)
    return [(int(a), int(b)) for a, b in s]


def substitute(read, p, rng):
    r = np.array(read, np.uint8).copy()
    others = [b for b in _ACGT if int(b) != int(r[p])]
    r[p] = others[int(rng.integers(0, len(others)))]
    return r


def both_strands(reads):
    """every second read as its reverse complement (it matches the reverse-strand copy of the contig)"""
    return [refdata.revcomp(r) if (i & 1) else r for i, r in enumerate(reads)]


def exact_reads(t, rng, L=L0, n_exons=24):
    """error-free reads: inside exons, flush with their first and last base, one base over each end, across short exons,
    from introns and from between the genes, from the first and last bases of the contig"""
    fwd = forward(t)
    n = len(fwd)
    ex = exons_forward(t)
    starts = []
    pick = [ex[i] for i in rng.permutation(len(ex))[:n_exons]]
    for a, b in pick:
        if b - a >= L:
            starts += [a, b - L, a - 1, b - L + 1, a + int(rng.integers(0, b - a - L + 1))]
        else:
            starts += [a - int(rng.integers(1, L - (b - a))), a - 1, b - L + 1]
    lo, hi = min(a for a, _ in ex), max(b for _, b in ex)
    starts += [int(v) for v in rng.integers(lo, hi - L, 40)]           # exons, introns, between the genes
    starts += [int(v) for v in rng.integers(max(hi, 0), n - L, 10)]   # behind the last gene
    starts += [0, 1, n - L, n - L - 1]
    reads = [fwd[s: s + L] for s in starts if 0 <= s <= n - L]
    reads = [r for r in reads if not (r == ord("N")).any()]
    return both_strands(reads)


def subst_reads(t, rng, L=L0, n_exons=16, ps=None):
    """reads inside exons, flush with their ends and 25 bases over them, with one substitution at p = 20, 21, 45, L - 22, L - 21;
    reads across an exon's end with the substitution on the exon's last or first base; intronic and intergenic ones"""
    fwd = forward(t)
    ex = [e for e in exons_forward(t) if e[1] - e[0] >= L]
    ps = ps or [20, 21, 45, L - 22, L - 21]
    reads = []
    for i in rng.permutation(len(ex))[:n_exons]:
        a, b = ex[i]
        for s in (a, b - L, a + int(rng.integers(0, b - a - L + 1)), a - 25, b - L + 25):
            if s < 0 or s + L > len(fwd) or (fwd[s: s + L] == ord("N")).any():
                continue
            for p in ps:
                reads.append(substitute(fwd[s: s + L], p, rng))
        # the substitution on the exon's last / first base, the read going on beyond it
        for s, p in ((b - 1 - L // 2, L // 2), (a - L // 2, L // 2)):
            if s >= 0 and s + L <= len(fwd) and not (fwd[s: s + L] == ord("N")).any():
                reads.append(substitute(fwd[s: s + L], p, rng))
    # intronic / intergenic ones
    lo, hi = min(a for a, _ in ex), max(b for _, b in ex)
    for s in rng.integers(lo, hi - L, 12):
        reads.append(substitute(fwd[int(s): int(s) + L], ps[int(rng.integers(0, len(ps)))], rng))
    return both_strands(reads)


def must_leave_reads(t, info, rng, L=L0):
    """reads the finisher must leave (planted_reference): an exact repeat, two SMEMs on different diagonals, a 1-base indel,
    N in the read, a read shorter than k, a flank of one repeated base and one of a two-letter repeat"""
    fwd = forward(t)
    a, b, _ = info["repeat"]
    e0, _ = info["exon"]
    reads = [fwd[a + 10: a + 10 + L], fwd[b + 30: b + 30 + L]]
    reads.append(np.concatenate([fwd[e0 + 10: e0 + 55], fwd[e0 + 60: e0 + 60 + L - 45]]))   # 5 bases missing: two diagonals
    r = fwd[e0 + 100: e0 + 100 + L + 1]
    reads.append(np.delete(r, 45))                                                         # a deleted base
    reads.append(np.insert(fwd[e0 + 100: e0 + 100 + L - 1], 45, _ACGT[0]))                 # an inserted base
    r = fwd[e0 + 20: e0 + 20 + L].copy()
    r[30] = ord("N")
    reads.append(r)
    reads.append(fwd[e0 + 20: e0 + 20 + 15])                                               # shorter than k
    h0, h1 = info["homopolymer"]
    r = fwd[h1 - L: h1].copy()          # the run of 21 is the read's right flank ...
    r[L - 22] = ord("A")                # ... and the substituted base in front of it repeats its base
    reads.append(r)
    r = fwd[h0: h0 + L].copy()          # the same on the left
    r[21] = ord("A")
    reads.append(r)
    d0, d1 = info["dinuc"]
    reads.append(substitute(fwd[d1 - L: d1], L - 23, rng))
    reads.append(substitute(fwd[d0: d0 + L], 22, rng))
    return both_strands(reads) + reads


def sanitise(bases):
    """what the pipeline's first kernel makes of the reads: upper case, bytes outside ACGTN -> 0"""
    b = np.array(bases, np.uint8).copy()
    low = (b >= ord("a")) & (b <= ord("z"))
    b[low] -= 32
    ok = np.isin(b, np.frombuffer(b"ACGTN", np.uint8))
    b[~ok] = 0
    return b


# ------------------------------------------------------------------ the host program
def fast_class(opts, lengths, limit=400):
    """(longest length of the fast class among `lengths`, its band, cells per lane) as extend_plan.h's classify() cuts it for
    reads of a few hundred bases (LDS is no limit there: lengths above `limit` are taken to be the slow class's)"""
    fast_len = fast_bw = 0
    for L in sorted(set(int(x) for x in lengths)):
        ms = max(int(np.float32(opts["min_aln_score_percent"]) * np.float32(L)), opts["min_aln_score"])
        bw = 0 if ms < 0 else max(L - ms, 0)
        if (2 * bw + 1 + 63) // 64 > 4 or L > limit:
            break
        fast_len, fast_bw = L, bw
    return fast_len, fast_bw, max(1, (2 * fast_bw + 1 + 63) // 64)


_exe = {}


def host_program(tmp_dir, sanitizers=False):
    key = bool(sanitizers)
    if key not in _exe:
        exe = os.path.join(str(tmp_dir), "smem_finish_main" + ("_san" if sanitizers else ""))
        extra = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if sanitizers else []
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra +
                              ["-I" + os.path.join(ROOT, "thermite_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "smem_finish_main.cpp"), "-o", exe])
        _exe[key] = exe
    return _exe[key]


def _pad8(b):
    return b + b"\0" * (-len(b) % 8)


def run_host(exe, w, opts, bases, off, tmp_dir, classes=CLASS_E | CLASS_S, tag="x"):
    """the header's decision for every read of the batch: a structured array (OUT_DT), and the op run's half length"""
    off = np.ascontiguousarray(off, "<u8")
    san = sanitise(bases)
    mems = w.oix.all_smems(san, off, opts["min_seed_len"])
    fast_len, fast_bw, cpl = fast_class(opts, np.diff(off.astype(np.int64)))
    half = fast_len
    blob = struct.pack("<IIII", 0x4E494653, w.ix.coord_bytes, len(w.t["refs"]), classes)
    for name in capi.Index.HOST_TABLES:
        tb = w.ix.debug_host_table(name).tobytes()
        blob += struct.pack("<Q", len(tb)) + _pad8(tb)
    blob += struct.pack("<QfiQii", opts["min_seed_len"], opts["min_aln_score_percent"], opts["min_aln_score"], opts["multimap_score_range"],
                        int(bool(opts["intron_mode"])), 0)
    blob += struct.pack("<IIII", fast_len, fast_bw, cpl, half)
    blob += struct.pack("<Q", len(off) - 1) + off.tobytes() + _pad8(san.tobytes())
    blob += np.ascontiguousarray(mems.offsets, "<u8").tobytes() + mems.mems.tobytes()
    fin, fout = os.path.join(str(tmp_dir), tag + ".in"), os.path.join(str(tmp_dir), tag + ".out")
    open(fin, "wb").write(blob)
    subprocess.run([exe, fin, fout], check=True)
    rows = np.loadtxt(fout, dtype=np.int64, ndmin=2)
    out = np.zeros(len(rows), OUT_DT)
    for k, f in enumerate(OUT_DT.names):
        out[f] = rows[:, k]
    assert len(out) == len(off) - 1
    return out, half


def finished_counts(out):
    """(class E finished, class E left, class S finished, class S left) as thm_debug_smem_finish_stats reports them"""
    return tuple(int(((out["shape"] == s) & (out["what"] == w)).sum()) for s in (1, 2) for w in (1, 0))


def assert_host_matches_oracle(w, opts, bases, off, out, half, per_read=96):
    """For every read the header finished: alignment record, op bytes and counter increments equal the oracle's.  The counters
    are compared in sum over all finished reads, and read by read (one oracle call each) for every finished read of a batch
    with up to 3 * per_read of them, else for per_read of them spread evenly over the batch."""
    off = np.asarray(off, np.int64)
    done = np.nonzero(out["what"] == 1)[0]
    if len(done) == 0:
        return 0
    reads = [np.asarray(bases[off[i]: off[i + 1]]) for i in done]
    sb, so = refdata.pack_reads(reads)
    r = w.oix.align_batch(sb, so, opts, n_threads=4)
    assert r.counters[15] == 0
    run = np.zeros(2 * half + 1, np.uint8)
    run[half] = 1
    ro = r.offsets.astype(np.int64)
    for j, i in enumerate(done):
        o, L = out[i], int(off[i + 1] - off[i])
        assert ro[j + 1] - ro[j] == o["accepted"], ("alignment count", int(i), o)
        if not o["accepted"]:
            continue
        a = r.alns[ro[j]]
        exonic = o["aln_type"] == EXONIC
        want = dict(ystart=o["ystart"], yend=o["yend"], ylen=o["ylen"], score=o["score"], ref_id=o["ref_id"], xstart=0, xend=L, xlen=L,
                    ops_len=L, tx_or_gene_idx=o["type_idx"], strand=o["strand"], aln_type=o["aln_type"], primary=1,
                    tx_ystart=o["tx_ystart"], tx_yend=o["tx_yend"], tx_ylen=o["tx_ylen"], tx_score=o["score"] if exonic else 0, tx_xstart=0,
                    tx_xend=L if exonic else 0, tx_ops_len=L if exonic else 0)
        for f, v in want.items():
            assert int(a[f]) == int(v), ("field " + f, int(i), a, o)
        assert np.array_equal(r.ops[int(a["ops_off"]): int(a["ops_off"]) + L], run[o["ops_off"]: o["ops_off"] + L]), ("genome ops", int(i))
        if exonic:
            assert np.array_equal(r.ops[int(a["tx_ops_off"]): int(a["tx_ops_off"]) + L], run[o["tx_ops_off"]: o["tx_ops_off"] + L]), ("tx ops", int(i))
        assert o["op_bytes"] == (2 * L if exonic else L)
    d = out[done]
    sums = (int(d["calls"].sum()), int(d["op_bytes"].sum()), int(d["window_bytes"].sum()), int(d["accepted"].sum()))
    assert sums == (int(r.counters[9]), int(r.counters[12]), int(r.counters[13]), int(r.counters[3])), (sums, r.counters[:14])
    pick = range(len(done)) if len(done) <= 3 * per_read else np.unique(np.linspace(0, len(done) - 1, per_read).astype(np.int64))
    for j in pick:
        i = done[j]
        r1 = w.oix.align_batch(reads[j], np.array([0, len(reads[j])], "<u8"), opts, n_threads=1)
        o = out[i]
        assert (int(r1.counters[9]), int(r1.counters[12]), int(r1.counters[13])) == (int(o["calls"]), int(o["op_bytes"]), int(o["window_bytes"])), \
            ("counters of read", int(i), r1.counters[:14], o)
    return len(done)


# ------------------------------------------------------------------ the finisher on the device
def check_device(exe, w, opts, reads, tmp_path, pool_caps=None, expect=None):
    """on the device (for tests marked gpu): check_align, then the three settings of the class switches with the finished / left
    counts of the host program -> (class E finished, class E left, class S finished, class S left) with both classes on"""
    import gpu_common as gc
    bases, off = reads if isinstance(reads, tuple) else refdata.pack_reads(reads)
    r = w.oix.align_batch(bases, off, opts, n_threads=8)
    gc.check_align(w, bases, off, opts, pool_caps=pool_caps, ref=r)
    counts = None
    for classes in (CLASS_E | CLASS_S, CLASS_E, CLASS_S):
        out, _ = run_host(exe, w, opts, bases, off, tmp_path, classes=classes, tag="c%d" % classes)
        a = w.aligner(opts)
        a.debug_set_flags(tpr=False, finish_exact=bool(classes & CLASS_E), finish_subst=bool(classes & CLASS_S))
        if pool_caps:
            a.debug_set_pool_caps(**pool_caps)
        a.reset_counters()
        g = a.align_batch(bases, off)
        gc.assert_batch_equal(g, r)
        gc.assert_counters_match(a.counters(), r.counters, classes)
        got, want = a.debug_smem_finish_stats(), finished_counts(out)
        assert got == want, (classes, got, want)
        if classes == (CLASS_E | CLASS_S):
            counts = want
            done = int(out["what"].sum())
            if expect == "all":
                assert done == len(off) - 1
                # finished reads add nothing to dp_cells and dp_cols: with every read finished both stay 0
                assert a.counters()[10] == 0 and a.counters()[11] == 0, a.counters()[:14]
            if expect == "none":
                assert done == 0
        a.close()
    return counts
