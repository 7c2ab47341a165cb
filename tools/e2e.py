#!/usr/bin/env python3
"""End-to-end file throughput on the GPU box (tuning aid, not the benchmark):
FASTQ on disk -> thm_align_files -> SAM / PAF.   python tools_e2e.py [ref_len] [n_reads] [threads] [rep]
--bam-device[=RUNS]: only FASTQ -> BAM and .fastq.gz -> BAM, each RUNS times (default 4) with THM_BAM_DEVICE 0, 1 and 2
in turn (the driver reads the switch at every call), in one session.
--fastq-device[=ROUNDS]: FASTQ -> BAM and two .fastq.gz -> BAM with THM_BAM_DEVICE 1 and 2, each with THM_FASTQ_DEVICE off
and on alternately, ROUNDS rounds (default 3) in one session; the files of a pair must be identical.
--fastq-bgzf[=ROUNDS]: the .fastq.gz files are written BGZF-framed with Python's zlib (level 6, members of 0xff00 bytes);
two of them -> BAM with THM_BAM_DEVICE 1 and 2, each with THM_FASTQ_DEVICE 1 and 2 alternately, ROUNDS rounds (default 3)
in one session; the inflated BAM streams of a pair must be identical (batch boundaries differ).
--fastq-gzip[=ROUNDS]: the `gzip -6` files as they are, one and two of them -> BAM with THM_BAM_DEVICE 1 and 2, each with
THM_FASTQ_DEVICE 1 and 3 alternately, ROUNDS rounds (default 3) in one session; the inflated BAM streams of a pair must be
identical (batch boundaries differ).
--bam-sort[=ROUNDS]: only plain FASTQ -> BAM with THM_FASTQ_DEVICE=1: THM_BAM_DEVICE=2 (input order), THM_BAM_SORT=1
(coordinate order) and THM_BAM_SORT=1 with THM_BAM_INDEX=1 (the .bai too; its size is reported) alternately, ROUNDS rounds
(default 3) in one session; then the same reads through thm_bam_sorter by hand: sort_ms of thm_bam_sorter_finish, the drain
with the two gather shapes alternating window by window (gather_ms, deflate_ms per window) and index_ms of
thm_bam_sorter_index, three calls.  The gzip files are not made.
--quant[=ROUNDS]: only plain FASTQ -> BAM with THM_BAM_DEVICE=1, without and with THM_QUANT=1 alternately, ROUNDS rounds
(default 3) in one session (the two .tsv files' sizes are reported); then one batch of 500 000 reads, of 91 and of 150
bases, through thm_quant by hand: add_ms and fetch_ms beside THM_T_CIGAR and THM_T_COMPACT of the same run, five adds each.
--coverage[=ROUNDS]: as --quant with THM_COVERAGE=3 (the bedGraph files' sizes are reported); then one batch of 500 000 reads,
of 91 and of 150 bases, through thm_coverage by hand: add_ms of five adds and fetch_ms of every track beside THM_T_CIGAR
and thm_quant_add's add_ms of the same run; then add_ms of 500 000 alignments of 50M at one position beside the same
number spread over the contig (the contention of the deposit's atomics).
--pileup[=ROUNDS]: as --quant with THM_PILEUP=1 (the .pileup.tsv's size is reported); then one batch of 500 000 reads, of 91
and of 150 bases, through thm_pileup by hand: add_ms of five adds (the first builds the table, the others find every row in
it), fetch_ms at min_alt 1 and 2, the ms of a window of 1 << 20 positions, n_events and the held bytes, beside
thm_coverage_add's and thm_quant_add's add_ms of the same run -- the two adds this one is made of.
--sha[=PART]: with any of the modes above, "sha256 <hash> <file> <bytes>" for every output file before it is removed (two
builds of the library -- THM_LIB selects one -- are compared by these lines); with PART also, after every run that wrote a
file whose name holds PART, "each <file> raw <hash> inflated <hash> size <bytes> batches <n>": does an output repeat from
run to run, compressed and inflated?"""
import hashlib, os, sys, time
BAM_RUNS = FQ_ROUNDS = BGZF_ROUNDS = GZIP_ROUNDS = SORT_ROUNDS = QUANT_ROUNDS = COV_ROUNDS = PILE_ROUNDS = 0
SHA, SHA_EACH = False, None
for arg in list(sys.argv[1:]):
    if arg.startswith("--sha"):
        SHA, SHA_EACH = True, (arg.split("=")[1] if "=" in arg else None)
        sys.argv.remove(arg)
        continue
    if arg.startswith("--pileup"):
        PILE_ROUNDS = int(arg.split("=")[1]) if "=" in arg else 3
        sys.argv.remove(arg)
        continue
    if arg.startswith("--coverage"):
        COV_ROUNDS = int(arg.split("=")[1]) if "=" in arg else 3
        sys.argv.remove(arg)
        continue
    if arg.startswith("--quant"):
        QUANT_ROUNDS = int(arg.split("=")[1]) if "=" in arg else 3
        sys.argv.remove(arg)
        continue
    if arg.startswith("--bam-sort"):
        SORT_ROUNDS = int(arg.split("=")[1]) if "=" in arg else 3
        sys.argv.remove(arg)
        continue
    if arg.startswith("--fastq-gzip"):
        GZIP_ROUNDS = int(arg.split("=")[1]) if "=" in arg else 3
        sys.argv.remove(arg)
        continue
    if arg.startswith("--fastq-bgzf"):
        BGZF_ROUNDS = int(arg.split("=")[1]) if "=" in arg else 3
        sys.argv.remove(arg)
        continue
    if arg.startswith("--fastq-device"):
        FQ_ROUNDS = int(arg.split("=")[1]) if "=" in arg else 3
        sys.argv.remove(arg)
        continue
    if arg.startswith("--bam-device"):
        BAM_RUNS = int(arg.split("=")[1]) if "=" in arg else 4
        sys.argv.remove(arg)
import numpy as np


def file_sha(p, opener=open):
    h = hashlib.sha256()
    with opener(p, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def drop(p):
    """removes a file of the tool's; an output file's hash first, with --sha"""
    if SHA and os.path.basename(p).startswith("thm_e2e_out"):
        print("sha256 %s %s %d" % (file_sha(p), p, os.path.getsize(p)), flush=True)
    os.remove(p)


sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thermite_amd import capi, synth

ref_len = int(sys.argv[1]) if len(sys.argv) > 1 else 4000000
n = int(sys.argv[2]) if len(sys.argv) > 2 else 2000000
threads = int(sys.argv[3]) if len(sys.argv) > 3 else 0
t = synth.synth_reference(length=ref_len)
ix = capi.Index(t)
bases, off, _ = synth.simulate_reads(t, n, 91, sub_rate=0.01, indel_rate=0.001, stream=100)
t0 = time.time()
path = "/tmp/thm_e2e_%d.fastq" % n
reads = bases.reshape(n, 91)
qual = np.full(91, ord("F"), np.uint8)
with open(path, "wb") as f:
    CH = 100000
    for s in range(0, n, CH):
        e = min(n, s + CH)
        parts = []
        for i in range(s, e):
            parts.append(b"@SYN:%d 1:N:0:ACGT\n" % i)
            parts.append(reads[i].tobytes())
            parts.append(b"\n+\n")
            parts.append(qual.tobytes())
            parts.append(b"\n")
        f.write(b"".join(parts))
print("fastq: %d reads, %.1f MB, written in %.1fs" % (n, os.path.getsize(path) / 1e6, time.time() - t0), flush=True)
a = capi.Aligner(ix, capi.CI_OPTS)
# the plain-FASTQ runs on a file of REP copies as well (a run over 2 M reads lasts 0.2 s: mostly first-touch of buffers)
REP = int(sys.argv[4]) if len(sys.argv) > 4 else 4
big = path + ".x%d" % REP
with open(big, "wb") as f:
    one = open(path, "rb").read()
    for _ in range(REP):
        f.write(one)
    del one
print("plain input: %d reads, %.1f MB" % (n * REP, os.path.getsize(big) / 1e6), flush=True)
if PILE_ROUNDS:
    os.environ["THM_BAM_DEVICE"] = "1"
    out = "/tmp/thm_e2e_out.bam"
    st = capi.align_files(a, [big], out, capi.FMT_BAM, batch_reads=250000, n_threads=threads)   # warm-up: buffers grow
    for k in range(PILE_ROUNDS):
        for tag, on in (("THM_BAM_DEVICE=1             ", False), ("THM_BAM_DEVICE=1 THM_PILEUP=1", True)):
            os.environ.pop("THM_PILEUP", None)
            if on:
                os.environ["THM_PILEUP"] = "1"
            st = capi.align_files(a, [big], out, capi.FMT_BAM, batch_reads=250000, n_threads=threads)
            tsv = ""
            if on:
                tsv = ", pileup.tsv %d bytes" % os.path.getsize(out + ".pileup.tsv")
                os.remove(out + ".pileup.tsv")
            print("bam %s round %d: %.2f Mreads/s wall %.3fs | parse %.2fs gpu %.2fs format %.2fs write %.2fs | %d batches, %.0f MB out%s" % (
                tag, k, st["n_reads"] / st["wall_s"] / 1e6, st["wall_s"], st["parse_s"], st["gpu_s"], st["format_s"], st["write_s"],
                st["n_batches"], st["n_output_bytes"] / 1e6, tsv), flush=True)
    os.environ.pop("THM_PILEUP", None)
    # one batch of 500 000 reads by hand
    for L in (91, 150):
        b, o, _ = synth.simulate_reads(t, 500000, L, sub_rate=0.01, indel_rate=0.001, stream=7)
        p = capi.Pileup(a, 0)
        c = capi.Coverage(a, 0)
        q = capi.Quant(a)
        a.upload(b, o)
        a.run()
        a.fetch_cigars(copy=False)
        tm = a.timings()
        adds = [p.add() for _ in range(5)]
        c_adds = [c.add() for _ in range(5)]
        q_adds = [q.add() for _ in range(5)]
        fetches = [[p.fetch(0, 1, m) for m in (1, 2)] for _ in range(3)]
        wins = [p.window(0, ref_len // 2, 1 << 20) for _ in range(3)]
        print("pileup %d bp: 500000 reads, %d alns, %d used, %d M bases, %d mismatches, %d del bases, %d ins | n_events %d, held %.1f MB | add_ms %s | "
              "fetch_ms min_alt 1, 2: %s | sites %d, %d | window_ms of 2^20 positions %s | thm_coverage_add add_ms %s | thm_quant_add add_ms %s | "
              "THM_T_CIGAR %.3f THM_T_COMPACT %.3f THM_T_TOTAL %.3f" % (
                  L, adds[0]["n_alns"], adds[0]["n_used_alns"], adds[0]["n_m_bases"], adds[0]["n_mismatches"], adds[0]["n_del_bases"], adds[0]["n_ins"],
                  adds[-1]["n_events"], adds[-1]["held_bytes"] / 1e6, " ".join("%.3f" % x["add_ms"] for x in adds),
                  " | ".join(" ".join("%.3f" % x.fetch_ms for x in f) for f in fetches), len(fetches[0][0].sites), len(fetches[0][1].sites),
                  " ".join("%.3f" % x.fetch_ms for x in wins), " ".join("%.3f" % x["add_ms"] for x in c_adds),
                  " ".join("%.3f" % x["add_ms"] for x in q_adds), tm["cigar"], tm["compact"], tm["total"]), flush=True)
        q.close()
        c.close()
        p.close()
    a.close()
    drop(out)
    sys.exit(0)
if COV_ROUNDS:
    import glob
    os.environ["THM_BAM_DEVICE"] = "1"
    out = "/tmp/thm_e2e_out.bam"
    st = capi.align_files(a, [big], out, capi.FMT_BAM, batch_reads=250000, n_threads=threads)   # warm-up: buffers grow
    for k in range(COV_ROUNDS):
        for tag, on in (("THM_BAM_DEVICE=1               ", False), ("THM_BAM_DEVICE=1 THM_COVERAGE=3", True)):
            os.environ.pop("THM_COVERAGE", None)
            if on:
                os.environ["THM_COVERAGE"] = "3"
            st = capi.align_files(a, [big], out, capi.FMT_BAM, batch_reads=250000, n_threads=threads)
            files = ""
            for f in sorted(glob.glob(out + ".cov.*.bedgraph")):
                files += ", %s %d bytes" % (f[len(out) + 5:], os.path.getsize(f))
                os.remove(f)
            print("bam %s round %d: %.2f Mreads/s wall %.3fs | parse %.2fs gpu %.2fs format %.2fs write %.2fs | %d batches, %.0f MB out%s" % (
                tag, k, st["n_reads"] / st["wall_s"] / 1e6, st["wall_s"], st["parse_s"], st["gpu_s"], st["format_s"], st["write_s"],
                st["n_batches"], st["n_output_bytes"] / 1e6, files), flush=True)
    os.environ.pop("THM_COVERAGE", None)
    # one batch of 500 000 reads by hand
    for L in (91, 150):
        b, o, _ = synth.simulate_reads(t, 500000, L, sub_rate=0.01, indel_rate=0.001, stream=7)
        c = capi.Coverage(a, capi.COV_STRANDED | capi.COV_MULTI)
        q = capi.Quant(a)
        a.upload(b, o)
        a.run()
        a.fetch_cigars(copy=False)
        tm = a.timings()
        adds = [c.add() for _ in range(5)]
        q_adds = [q.add() for _ in range(5)]
        fetches = [[c.fetch(k, 0, 1) for k in range(4)] for _ in range(3)]
        depth_ms = []
        for _ in range(3):
            c.depth(0, 0, ref_len // 2, 1 << 20)
            depth_ms.append(c.depth_ms)
        tr = adds[0]["track"]
        print("coverage %d bp: 500000 reads, %d alns, %d blocks, %d bases, held %.1f MB | add_ms %s | fetch_ms per track %s | runs per track %s, max depth %d | "
              "depth_ms of 2^20 bases %s | thm_quant_add add_ms %s | THM_T_CIGAR %.3f THM_T_COMPACT %.3f THM_T_TOTAL %.3f" % (
                  L, adds[0]["n_alns"], sum(x["n_blocks"] for x in tr), sum(x["n_bases"] for x in tr), adds[0]["held_bytes"] / 1e6,
                  " ".join("%.3f" % x["add_ms"] for x in adds), " | ".join(" ".join("%.3f" % x.fetch_ms for x in f) for f in fetches),
                  " ".join("%d" % len(x.runs) for x in fetches[0]), max(x.max_depth for x in fetches[0]),
                  " ".join("%.3f" % x for x in depth_ms), " ".join("%.3f" % x["add_ms"] for x in q_adds), tm["cigar"], tm["compact"], tm["total"]), flush=True)
        q.close()
        c.close()
    # the contention of the deposit: every alignment on one position, and the same number spread out
    N = 500000
    fwd_ref = int(np.nonzero(t["refs"]["strand"] == 1)[0][0])
    rng = np.random.default_rng(11)
    for tag, ystart in (("hot   ", np.full(N, ref_len // 3, np.uint64)), ("spread", rng.integers(0, ref_len - 100, N).astype(np.uint64))):
        alns = np.zeros(N, capi.ALN_DT)
        alns["ystart"], alns["ref_id"], alns["aln_type"], alns["tx_or_gene_idx"], alns["strand"] = ystart, fwd_ref, 2, 0xFFFFFFFF, 1
        dig = np.zeros(N, capi.DIGEST_DT)
        dig["cigar_off"], dig["n_cigar"], dig["ref_len"] = np.arange(N, dtype=np.uint64), 1, 50
        words = np.full(N, 50 << 4, "<u4")
        c = capi.Coverage(a, 0)
        adds = [c.add_view(np.arange(N + 1, dtype="<u8"), alns, dig, words) for _ in range(5)]
        res = c.fetch(0, 0, 1)
        print("deposit %s: %d alignments of 50M, %d runs, max depth %d | add_ms %s | fetch_ms %.3f" % (
            tag, N, len(res.runs), res.max_depth, " ".join("%.3f" % x["add_ms"] for x in adds), res.fetch_ms), flush=True)
        c.close()
    a.close()
    drop(out)
    sys.exit(0)
if QUANT_ROUNDS:
    os.environ["THM_BAM_DEVICE"] = "1"
    out = "/tmp/thm_e2e_out.bam"
    st = capi.align_files(a, [big], out, capi.FMT_BAM, batch_reads=250000, n_threads=threads)   # warm-up: buffers grow
    for k in range(QUANT_ROUNDS):
        for tag, on in (("THM_BAM_DEVICE=1            ", False), ("THM_BAM_DEVICE=1 THM_QUANT=1", True)):
            os.environ.pop("THM_QUANT", None)
            if on:
                os.environ["THM_QUANT"] = "1"
            st = capi.align_files(a, [big], out, capi.FMT_BAM, batch_reads=250000, n_threads=threads)
            tsv = ""
            if on:
                tsv = ", genes.tsv %d bytes, junctions.tsv %d bytes" % (os.path.getsize(out + ".genes.tsv"), os.path.getsize(out + ".junctions.tsv"))
                os.remove(out + ".genes.tsv")
                os.remove(out + ".junctions.tsv")
            print("bam %s round %d: %.2f Mreads/s wall %.3fs | parse %.2fs gpu %.2fs format %.2fs write %.2fs | %d batches, %.0f MB out%s" % (
                tag, k, st["n_reads"] / st["wall_s"] / 1e6, st["wall_s"], st["parse_s"], st["gpu_s"], st["format_s"], st["write_s"],
                st["n_batches"], st["n_output_bytes"] / 1e6, tsv), flush=True)
    os.environ.pop("THM_QUANT", None)
    # one batch of 500 000 reads by hand
    for L in (91, 150):
        b, o, _ = synth.simulate_reads(t, 500000, L, sub_rate=0.01, indel_rate=0.001, stream=7)
        q = capi.Quant(a)
        a.upload(b, o)
        a.run()
        a.fetch_cigars(copy=False)
        tm = a.timings()
        adds = [q.add() for _ in range(5)]
        fetches = [q.fetch() for _ in range(3)]
        print("quant %d bp: 500000 reads, %d alns, %d spliced, %d hits -> %d junctions, held %.1f MB | add_ms %s | fetch_ms %s | THM_T_CIGAR %.3f THM_T_COMPACT %.3f THM_T_TOTAL %.3f" % (
            L, adds[0]["n_alns"], adds[0]["n_spliced_alns"], adds[0]["n_junction_hits"], adds[0]["n_junctions"], adds[0]["held_bytes"] / 1e6,
            " ".join("%.3f" % x["add_ms"] for x in adds), " ".join("%.3f" % x.fetch_ms for x in fetches), tm["cigar"], tm["compact"], tm["total"]), flush=True)
        q.close()
    a.close()
    drop(out)
    sys.exit(0)
if SORT_ROUNDS:
    os.environ["THM_FASTQ_DEVICE"] = "1"
    os.environ["THM_BAM_DEVICE"] = "2"
    st = capi.align_files(a, [big], "/tmp/thm_e2e_out.bam", capi.FMT_BAM, batch_reads=250000, n_threads=threads)   # warm-up: buffers grow
    for k in range(SORT_ROUNDS):
        for tag, env in (("input order, THM_BAM_DEVICE=2", {"THM_BAM_DEVICE": "2"}), ("sorted,      THM_BAM_SORT=1  ", {"THM_BAM_SORT": "1"}),
                         ("sorted + .bai, THM_BAM_INDEX=1", {"THM_BAM_SORT": "1", "THM_BAM_INDEX": "1"})):
            for name in ("THM_BAM_DEVICE", "THM_BAM_SORT", "THM_BAM_INDEX"):
                os.environ.pop(name, None)
            os.environ.update(env)
            st = capi.align_files(a, [big], "/tmp/thm_e2e_out.bam", capi.FMT_BAM, batch_reads=250000, n_threads=threads)
            bai = ""
            if "THM_BAM_INDEX" in env:
                bai = ", .bai %.2f MB" % (os.path.getsize("/tmp/thm_e2e_out.bam.bai") / 1e6)
                os.remove("/tmp/thm_e2e_out.bam.bai")
            print("bam %s round %d: %.2f Mreads/s wall %.2fs | parse %.2fs gpu %.2fs format %.2fs write %.2fs | %d records, %.0f MB out%s" % (
                tag, k, st["n_reads"] / st["wall_s"] / 1e6, st["wall_s"], st["parse_s"], st["gpu_s"], st["format_s"], st["write_s"],
                st["n_records"], st["n_output_bytes"] / 1e6, bai), flush=True)
    os.environ.pop("THM_BAM_SORT", None)
    os.environ.pop("THM_BAM_INDEX", None)
    # the sorter by hand: add every batch, sort, drain with the gather shapes alternating
    W = 256 * 0xff00
    for rnd in range(2):
        rd = capi.FastqReader(big)
        srt = capi.BamSorter(a)
        t0 = time.perf_counter()
        add_ms = []
        while True:
            batch = rd.next_batch(250000)
            if batch is None or len(batch["offsets"]) <= 1:
                break
            a.upload_reads(batch)
            a.run()
            add_ms.append(srt.add()["add_ms"])
        rd.close()
        t_add = time.perf_counter() - t0
        t0 = time.perf_counter(); sort_ms = srt.finish(); t_fin = time.perf_counter() - t0
        per, defl, k, total = {"pieces": [], "records": []}, [], 0, 0
        t0 = time.perf_counter()
        while True:
            shape = ("pieces", "records")[(k + rnd) & 1]
            srt.gather_shape(shape)
            v = srt.next(0, copy=False)
            if v.n_raw_bytes == 0:
                break
            total = v.total_raw_bytes
            if v.n_raw_bytes == W:
                per[shape].append(v.gather_ms)
                defl.append(v.deflate_ms)
            k += 1
        t_drain = time.perf_counter() - t0
        print("sorter round %d: %d batches added in %.2fs (add_ms median %.3f); finish: %d records, sort_ms %.2f, call %.3fs; drain: %d windows, %.0f MB of records in %.2fs" % (
            rnd, len(add_ms), t_add, float(np.median(add_ms)), v.total_records, sort_ms, t_fin, k, total / 1e6, t_drain), flush=True)
        for shape, ms in per.items():
            print("  gather[%-7s] %d windows of %d bytes: median %.3f ms (min %.3f max %.3f) = %.2f TB/s read+written" % (
                shape, len(ms), W, float(np.median(ms)), min(ms), max(ms), 2 * W / (float(np.median(ms)) * 1e-3) / 1e12), flush=True)
        print("  deflate per window: median %.3f ms (min %.3f max %.3f)" % (float(np.median(defl)), min(defl), max(defl)), flush=True)
        ims = [srt.index(1000) for _ in range(3)]
        print("  index: %d bytes, %d bins, %d chunks, %d windows: index_ms %s (sort_ms %.2f)" % (
            len(ims[0][0]), ims[0][1]["n_bins"], ims[0][1]["n_chunks"], ims[0][1]["n_intervals"], " ".join("%.2f" % x[1]["index_ms"] for x in ims), sort_ms), flush=True)
        srt.close()
    a.close()
    drop("/tmp/thm_e2e_out.bam")
    sys.exit(0)
for fmt, name in (() if BAM_RUNS or FQ_ROUNDS or BGZF_ROUNDS or GZIP_ROUNDS else ((capi.FMT_SAM, "sam"), (capi.FMT_PAF, "paf"))):
    for rep in range(2):
        out = "/tmp/thm_e2e_out.%s" % name
        st = capi.align_files(a, [big], out, fmt, batch_reads=250000, n_threads=threads)
        print("%s run %d: %.2f Mreads/s wall %.2fs | parse %.2fs gpu %.2fs format %.2fs write %.2fs | %d batches, %.0f MB out" % (
            name, rep, st["n_reads"] / st["wall_s"] / 1e6, st["wall_s"], st["parse_s"], st["gpu_s"], st["format_s"], st["write_s"],
            st["n_batches"], st["n_output_bytes"] / 1e6), flush=True)
# gzip input (the reference's own input format, src/aligner.rs:51-52): one file, then two files (an inflater thread each)
import gzip, shutil, subprocess
gz = path + ".gz"
t0 = time.time()
if BGZF_ROUNDS:
    import struct, zlib
    with open(path, "rb") as fi, open(gz, "wb") as fo:
        for piece in iter(lambda: fi.read(0xff00), b""):
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            z = c.compress(piece) + c.flush()
            fo.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(z) + 25) + z +
                     struct.pack("<II", zlib.crc32(piece), len(piece)))
elif shutil.which("gzip"):
    subprocess.check_call("gzip -6 -c %s > %s" % (path, gz), shell=True)
else:
    with open(path, "rb") as fi, gzip.open(gz, "wb", compresslevel=6) as fo:
        shutil.copyfileobj(fi, fo, 1 << 24)
print("gzip -6: %.1f MB in %.1fs" % (os.path.getsize(gz) / 1e6, time.time() - t0), flush=True)
# longer inputs without waiting for gzip: REP copies of the member back to back (a valid gzip file; `cat a.gz a.gz`)
if REP > 1:
    one = open(gz, "rb").read()
    with open(gz, "wb") as f:
        for _ in range(REP):
            f.write(one)
    del one
gz2 = path + ".2.gz"
shutil.copyfile(gz, gz2)
try:
    quota = open("/sys/fs/cgroup/cpu.max").read().strip()
except OSError:
    quota = "?"
print("each .gz: %d reads in %d member(s), %.1f MB; host: %d hardware threads, cpu.max %s" % (n * REP, REP, os.path.getsize(gz) / 1e6, os.cpu_count(), quota), flush=True)


def digest(path):
    import hashlib
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


paf_of_plain = None if BAM_RUNS or FQ_ROUNDS or BGZF_ROUNDS or GZIP_ROUNDS else digest("/tmp/thm_e2e_out.paf")  # (the last plain run wrote PAF of the REP-copy file)


def run(tag, paths, fmt, out, reps=2):
    for rep in range(reps):
        st = capi.align_files(a, paths, out, fmt, batch_reads=250000, n_threads=threads)
        print("%s run %d: %.2f Mreads/s wall %.2fs | parse+inflate %.2fs gpu %.2fs format %.2fs write %.2fs | %.0f MB out" % (
            tag, rep, st["n_reads"] / st["wall_s"] / 1e6, st["wall_s"], st["parse_s"], st["gpu_s"], st["format_s"], st["write_s"],
            st["n_output_bytes"] / 1e6), flush=True)
        if SHA_EACH and SHA_EACH in os.path.basename(out):
            print("each %s raw %s inflated %s size %d batches %d" % (out, file_sha(out), file_sha(out, gzip.open), os.path.getsize(out), st["n_batches"]), flush=True)


def inflated_sha(p):
    import hashlib
    h = hashlib.sha256()
    with gzip.open(p, "rb") as f:
        for blk in iter(lambda: f.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


if BGZF_ROUNDS:
    os.environ["THM_BAM_DEVICE"] = "1"
    os.environ["THM_FASTQ_DEVICE"] = "1"
    run("warm-up: bam from two BGZF .gz, THM_BAM_DEVICE=1, THM_FASTQ_DEVICE=1", [gz, gz2], capi.FMT_BAM, "/tmp/thm_e2e_out.bam", 1)
    outs, same = [], True
    for k in range(BGZF_ROUNDS):
        for dev in ("1", "2"):
            os.environ["THM_BAM_DEVICE"] = dev
            pair = []
            for fq in ("1", "2"):
                os.environ["THM_FASTQ_DEVICE"] = fq
                out = "/tmp/thm_e2e_out.z%s%s.bam" % (dev, fq)
                before = a.debug_fastq_bgzf_blocks()
                run("bam from two BGZF .gz, THM_BAM_DEVICE=%s, THM_FASTQ_DEVICE=%s, round %d" % (dev, fq, k), [gz, gz2], capi.FMT_BAM, out, 1)
                after = a.debug_fastq_bgzf_blocks()
                if fq == "2":
                    print("    groups inflated on the device %d, on the host %d; parsed on the device %d, on the host %d" % tuple(
                        y - x for x, y in zip(before, after)), flush=True)
                if k == 0:
                    pair.append(inflated_sha(out))
                outs.append(out)
            same = same and (k > 0 or pair[0] == pair[1])
    print("inflated BAM streams with THM_FASTQ_DEVICE 1 and 2 are %s" % ("IDENTICAL" if same else "DIFFERENT"), flush=True)
    a.close()
    for f in [path, big, gz, gz2, "/tmp/thm_e2e_out.bam"] + outs:
        if os.path.exists(f):
            drop(f)
    assert same
    sys.exit(0)
if GZIP_ROUNDS:
    os.environ["THM_BAM_DEVICE"] = "1"
    os.environ["THM_FASTQ_DEVICE"] = "1"
    run("warm-up: bam from two .gz, THM_BAM_DEVICE=1, THM_FASTQ_DEVICE=1", [gz, gz2], capi.FMT_BAM, "/tmp/thm_e2e_out.bam", 1)
    outs, same = [], True
    for k in range(GZIP_ROUNDS):
        for files in ([gz], [gz, gz2]):
            for dev in ("1", "2"):
                os.environ["THM_BAM_DEVICE"] = dev
                pair = []
                for fq in ("1", "3"):
                    os.environ["THM_FASTQ_DEVICE"] = fq
                    out = "/tmp/thm_e2e_out.g%d%s%s.bam" % (len(files), dev, fq)
                    before = a.debug_fastq_gzip_blocks()
                    run("bam from %d gzip -6 .gz, THM_BAM_DEVICE=%s, THM_FASTQ_DEVICE=%s, round %d" % (len(files), dev, fq, k), files, capi.FMT_BAM, out, 1)
                    after = a.debug_fastq_gzip_blocks()
                    if fq == "3":
                        print("    slices inflated on the device %d, on the host %d; parsed on the device %d, on the host %d" % tuple(
                            y - x for x, y in zip(before, after)), flush=True)
                    if k == 0:
                        pair.append(inflated_sha(out))
                    outs.append(out)
                same = same and (k > 0 or pair[0] == pair[1])
    print("inflated BAM streams with THM_FASTQ_DEVICE 1 and 3 are %s" % ("IDENTICAL" if same else "DIFFERENT"), flush=True)
    a.close()
    for f in [path, big, gz, gz2, "/tmp/thm_e2e_out.bam"] + outs:
        if os.path.exists(f):
            drop(f)
    assert same
    sys.exit(0)
if FQ_ROUNDS:
    os.environ["THM_BAM_DEVICE"] = "1"
    os.environ.pop("THM_FASTQ_DEVICE", None)
    run("warm-up: bam from plain fastq, device encoder, host parser", [big], capi.FMT_BAM, "/tmp/thm_e2e_out.bam", 1)
    outs, same = [], True
    for k in range(FQ_ROUNDS):
        for dev in ("1", "2"):
            os.environ["THM_BAM_DEVICE"] = dev
            for tag, paths in (("plain fastq", [big]), ("two .gz", [gz, gz2])):
                pair = []
                for fq in ("0", "1"):
                    os.environ["THM_FASTQ_DEVICE"] = fq
                    out = "/tmp/thm_e2e_out.fq%s%s%d.bam" % (dev, fq, len(paths))
                    before = a.debug_fastq_device_blocks()
                    run("bam from %s, THM_BAM_DEVICE=%s, %s parser, round %d" % (tag, dev, "device" if fq == "1" else "host  ", k), paths, capi.FMT_BAM, out, 1)
                    after = a.debug_fastq_device_blocks()
                    if fq == "1":
                        print("    blocks parsed on the device %d, on the host %d" % (after[0] - before[0], after[1] - before[1]), flush=True)
                    pair.append(digest(out))
                    outs.append(out)
                same = same and pair[0] == pair[1]
    print("BAM files with and without THM_FASTQ_DEVICE are %s" % ("IDENTICAL" if same else "DIFFERENT"), flush=True)
    a.close()
    for f in [path, big, gz, gz2, "/tmp/thm_e2e_out.bam"] + outs:
        if os.path.exists(f):
            drop(f)
    assert same
    sys.exit(0)
if BAM_RUNS:
    os.environ.pop("THM_BAM_DEVICE", None)
    run("warm-up: bam from plain fastq, host encoder", [big], capi.FMT_BAM, "/tmp/thm_e2e_out.bam", 1)
    sums = {}
    for k in range(BAM_RUNS):
        for dev in ("0", "1", "2"):
            os.environ["THM_BAM_DEVICE"] = dev
            what = {"0": "host encoder", "1": "device encoder", "2": "device encoder and deflate"}[dev]
            run("bam from plain fastq, %s, round %d" % (what, k), [big], capi.FMT_BAM, "/tmp/thm_e2e_out.%s.bam" % dev, 1)
            run("bam from two .gz, %s, round %d" % (what, k), [gz, gz2], capi.FMT_BAM, "/tmp/thm_e2e_out.gz%s.bam" % dev, 1)
    same = digest("/tmp/thm_e2e_out.0.bam") == digest("/tmp/thm_e2e_out.1.bam") and digest("/tmp/thm_e2e_out.gz0.bam") == digest("/tmp/thm_e2e_out.gz1.bam")
    print("BAM files of the two encoders are %s" % ("IDENTICAL" if same else "DIFFERENT"), flush=True)

    def inflated_digest(p):
        import hashlib
        h = hashlib.sha256()
        with gzip.open(p, "rb") as f:
            for blk in iter(lambda: f.read(1 << 24), b""):
                h.update(blk)
        return h.hexdigest()

    # the device's members are other bytes than the host's blocks: the files are compared inflated
    same2 = inflated_digest("/tmp/thm_e2e_out.2.bam") == inflated_digest("/tmp/thm_e2e_out.0.bam")
    print("BAM file of the device deflate inflates to %s; %d bytes against %d" % ("THE SAME BYTES" if same2 else "OTHER BYTES", os.path.getsize("/tmp/thm_e2e_out.2.bam"),
                                                                                 os.path.getsize("/tmp/thm_e2e_out.0.bam")), flush=True)
    same = same and same2
    a.close()
    for f in (path, big, gz, gz2, "/tmp/thm_e2e_out.bam", "/tmp/thm_e2e_out.0.bam", "/tmp/thm_e2e_out.1.bam", "/tmp/thm_e2e_out.2.bam", "/tmp/thm_e2e_out.gz0.bam",
              "/tmp/thm_e2e_out.gz1.bam", "/tmp/thm_e2e_out.gz2.bam"):
        if os.path.exists(f):
            drop(f)
    assert same
    sys.exit(0)
run("paf from one .gz", [gz], capi.FMT_PAF, "/tmp/thm_e2e_out.paf")
# the .gz holds the same records as the plain file (REP members of the same reads): same PAF, byte for byte
same = digest("/tmp/thm_e2e_out.paf") == paf_of_plain
print("PAF of the .gz input %s the PAF of the plain input (sha256 over %d reads)" % ("EQUALS" if same else "DIFFERS FROM", n * REP), flush=True)
assert same
run("paf from two .gz", [gz, gz2], capi.FMT_PAF, "/tmp/thm_e2e_out.paf")
run("bam from plain fastq", [big], capi.FMT_BAM, "/tmp/thm_e2e_out.bam")
run("bam from two .gz", [gz, gz2], capi.FMT_BAM, "/tmp/thm_e2e_out.bam")
a.close()
for f in (path, big, gz, gz2, "/tmp/thm_e2e_out.sam", "/tmp/thm_e2e_out.paf", "/tmp/thm_e2e_out.bam"):
    if os.path.exists(f):
        drop(f)
