#!/usr/bin/env python3
"""Quick stage timing on the GPU box (tuning aid, not the benchmark):
python tools/perf.py [ref_len] [n_reads] [opts] [--cigars] [--bam] [--bgzf] [--bam-sort] [--fastq] [--fastq-bgzf] [--fastq-gzip]
--cigars: on the resident batch, thm_batch_fetch against thm_batch_fetch_cigars -- milliseconds and bytes moved to the
host by each, and the device time of the two CIGAR passes (THM_T_CIGAR).
--bam: on the resident batch, thm_batch_fetch_bam with both forms of the emit kernel (THM_BAM_EMIT) -- milliseconds,
bytes, THM_T_BAM -- beside thm_batch_fetch plus the host's record encoding of the same batch (thm_writer_format_batch
at THM_BAM_LEVEL=0 minus thm_writer_wrap_bam of the same records: stored blocks, so the difference is the encoding).
--bgzf (without --bam, which turns the host's deflate off): on the resident batch, thm_batch_fetch_bgzf -- milliseconds,
bytes, THM_T_BGZF -- beside thm_batch_fetch_bam plus thm_writer_wrap_bam of the same records on 16 threads and on 1, and
the compressed sizes of the device encoder, the host encoder and zlib level 1 over the device's cuts.
--bam-sort: on the resident batch, thm_bam_sorter_add (the records stay on the device) against thm_batch_fetch_bam (they
cross to the host), alternately in one session -- milliseconds of the calls and add_ms (key kernel + copy) -- then
thm_bam_sorter_finish over everything added (sort_ms), the drain with the two gather shapes alternating window by window and
thm_bam_sorter_index over the drained stream (index_ms).
--fastq: the batch written out as one FASTQ block: thm_batch_upload_fastq -- milliseconds of the call and of its parse
kernels (device_ms) -- beside thm_batch_upload_reads of the parsed batch, and the host's parse of the block on one thread.
--fastq-bgzf: the same block BGZF-framed with Python's zlib (level 6, members of 0xff00 bytes): thm_batch_upload_fastq_bgzf
-- milliseconds of the call, of its inflate kernel (inflate_ms) and of its parse kernels (parse_ms) -- beside
thm_batch_upload_fastq of the inflated bytes and zlib's inflate of the members on one host thread.
--fastq-gzip: the same block as ONE gzip member (zlib level 6): thm_batch_upload_fastq_gzip -- milliseconds of the call, of
its inflate kernels (inflate_ms) and of its parse kernels (parse_ms), chunks, starts and the starts the chain refused --
beside thm_batch_upload_fastq of the inflated bytes and zlib's inflate of the member on one host thread; then the same
with varied qualities (the tool's all-F lines are kind to a decoder).  THM_GZIP_CHUNK_KB sets the chunk size."""
import sys, time
import numpy as np
sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from thermite_amd import capi, synth

cigars = "--cigars" in sys.argv
bam = "--bam" in sys.argv
bgzf = "--bgzf" in sys.argv
bam_sort = "--bam-sort" in sys.argv
fastq = "--fastq" in sys.argv
fastq_bgzf = "--fastq-bgzf" in sys.argv
fastq_gzip = "--fastq-gzip" in sys.argv
sys.argv = [x for x in sys.argv if x not in ("--cigars", "--bam", "--bgzf", "--bam-sort", "--fastq", "--fastq-bgzf", "--fastq-gzip")]
if bam:
    __import__("os").environ["THM_BAM_LEVEL"] = "0"  # (read once, by the first BGZF block of the process)
ref_len = int(sys.argv[1]) if len(sys.argv) > 1 else 4000000
n = int(sys.argv[2]) if len(sys.argv) > 2 else 500000
which = sys.argv[3] if len(sys.argv) > 3 else "both"
t = synth.synth_reference(length=ref_len)
ix = capi.Index(t)
bases, off, _ = synth.simulate_reads(t, n, 91, sub_rate=0.01, indel_rate=0.001, stream=100)
for name, opts in (("ci", capi.CI_OPTS), ("default", capi.DEFAULT_OPTS)):
    if which not in ("both", name):
        continue
    a = capi.Aligner(ix, opts)
    a.upload(bases, off)
    for _ in range(2):
        a.run(); a.sync()
    acc = {}
    K = 5
    t0 = time.perf_counter()
    for _ in range(K):
        a.run(); a.sync()
        for k, v in a.timings().items():
            acc[k] = acc.get(k, 0.0) + v / K
    dt = (time.perf_counter() - t0) / K
    print("%-8s ref=%d n=%d  %.2f Mreads/s  wall %.2f ms  " % (name, ref_len, n, n / dt / 1e6, dt * 1e3) +
          " ".join("%s=%.2f" % kv for kv in acc.items()), flush=True)
    if cigars:
        K2 = 7
        for fetch in (a.fetch, a.fetch_cigars, a.fetch, a.fetch_cigars):   # first round: buffers grow
            ms = []
            for _ in range(K2):
                t0 = time.perf_counter()
                r = fetch(copy=False)
                ms.append((time.perf_counter() - t0) * 1e3)
        for nm, fetch in (("fetch", a.fetch), ("fetch_cigars", a.fetch_cigars)):
            ms = []
            for _ in range(K2):
                t0 = time.perf_counter()
                r = fetch(copy=False)
                ms.append((time.perf_counter() - t0) * 1e3)
            nbytes = sum(x.nbytes for x in (r.offsets, r.alns, getattr(r, "ops", None), getattr(r, "digests", None),
                                            getattr(r, "cigar", None), r.status) if x is not None)
            extra = "" if nm == "fetch" else "  words %d  THM_T_CIGAR %.3f ms" % (len(r.cigar), a.timings()["cigar"])
            print("         %-12s median %.2f ms (min %.2f max %.2f, %d calls)  %d bytes to the host  alns %d%s" % (
                nm, float(np.median(ms)), min(ms), max(ms), K2, nbytes, len(r.alns), extra), flush=True)
    if bam:
        import os
        K2 = 7
        names = [b"SYN:%d 1:N:0:ACGT" % i for i in range(n)]
        batch = dict(bases=bases, offsets=off, quals=np.full(len(bases), ord("F"), np.uint8), names=np.frombuffer(b"".join(names), np.uint8),
                     name_off=np.cumsum([0] + [len(x) for x in names]).astype("<u8"))

        def med(f):
            ms = []
            for _ in range(K2):
                t0 = time.perf_counter()
                r = f()
                ms.append((time.perf_counter() - t0) * 1e3)
            return r, float(np.median(ms)), min(ms), max(ms)

        recs = None
        for form in ("bytes", "dwords", "bytes", "dwords"):   # first round: buffers grow
            os.environ["THM_BAM_EMIT"] = form
            b = capi.Aligner(ix, opts)
            b.upload_reads(batch)
            b.run(); b.sync()
            b.fetch_bam(copy=False)
            tb = []
            for _ in range(K2):
                b.fetch_bam(copy=False)
                tb.append(b.timings()["bam"])
            g, m, lo, hi = med(lambda: b.fetch_bam(copy=False))
            print("         fetch_bam[%-6s] median %.2f ms (min %.2f max %.2f)  %d bytes to the host  records %d  THM_T_BAM median %.3f ms (min %.3f max %.3f)" % (
                form, m, lo, hi, g.nbytes, g.n_records, float(np.median(tb)), min(tb), max(tb)), flush=True)
            recs = capi.BamResult.__new__(capi.BamResult)
            recs.data, recs.read_rec_off, recs.n_records = g.data.copy(), g.read_rec_off.copy(), g.n_records
            f, m, lo, hi = med(lambda: b.fetch(copy=False))
            full = (f.offsets.copy(), f.alns.copy(), f.ops.copy())
            print("         fetch          median %.2f ms (min %.2f max %.2f)  %d bytes to the host" % (m, lo, hi, sum(x.nbytes for x in full)), flush=True)
            b.close()
        os.environ.pop("THM_BAM_EMIT", None)
        res = capi.BatchResult.__new__(capi.BatchResult)
        res.offsets, res.alns, res.ops = full
        for threads in (16, 1):
            w = capi.Writer(ix, capi.FMT_BAM, n_threads=threads)
            w.format_batch(batch, res)
            o1, m1, lo1, hi1 = med(lambda: w.format_batch(batch, res))
            o2, m2, lo2, hi2 = med(lambda: w.wrap_bam(recs))
            print("         host, %2d threads: format_batch (encode + stored blocks) median %.2f ms (min %.2f max %.2f); wrap_bam (stored blocks only) "
                  "median %.2f ms (min %.2f max %.2f); encoding = %.2f ms; outputs %s" % (threads, m1, lo1, hi1, m2, lo2, hi2, m1 - m2,
                                                                                         "equal" if o1 == o2 else "DIFFER"), flush=True)
            w.close()
    if bam_sort:
        K2 = 7
        names = [b"SYN:%d 1:N:0:ACGT" % i for i in range(n)]
        batch = dict(bases=bases, offsets=off, quals=np.full(len(bases), ord("F"), np.uint8), names=np.frombuffer(b"".join(names), np.uint8),
                     name_off=np.cumsum([0] + [len(x) for x in names]).astype("<u8"))
        b = capi.Aligner(ix, opts)
        b.upload_reads(batch)
        b.run(); b.sync()
        srt = capi.BamSorter(b)
        for _ in range(2):   # buffers grow
            srt.add()
            b.fetch_bam(copy=False)
        ma, mk, mg = [], [], []
        for _ in range(K2):   # alternately, in one session
            t0 = time.perf_counter(); info = srt.add(); ma.append((time.perf_counter() - t0) * 1e3); mk.append(info["add_ms"])
            t0 = time.perf_counter(); g = b.fetch_bam(copy=False); mg.append((time.perf_counter() - t0) * 1e3)
        print("         sorter_add  median %.2f ms (min %.2f max %.2f, %d calls)  %d bytes stay on the device  add_ms median %.3f (min %.3f max %.3f)" % (
            float(np.median(ma)), min(ma), max(ma), K2, info["n_bytes"], float(np.median(mk)), min(mk), max(mk)), flush=True)
        print("         fetch_bam   median %.2f ms (min %.2f max %.2f, %d calls)  %d bytes to the host" % (float(np.median(mg)), min(mg), max(mg), K2, g.nbytes), flush=True)
        t0 = time.perf_counter(); sort_ms = srt.finish(); wall = (time.perf_counter() - t0) * 1e3
        print("         finish: %d records, %d bytes: sort_ms %.2f, call %.2f ms" % (info["total_records"], info["total_bytes"], sort_ms, wall), flush=True)
        per = {"pieces": [], "records": []}
        defl, k, t0 = [], 0, time.perf_counter()
        while True:
            shape = ("pieces", "records")[k & 1]
            srt.gather_shape(shape)
            v = srt.next(0, copy=False)
            if v.n_raw_bytes == 0:
                break
            if v.n_raw_bytes == 256 * 0xff00:
                per[shape].append(v.gather_ms)
                defl.append(v.deflate_ms)
            k += 1
        wall = time.perf_counter() - t0
        for shape, ms in per.items():
            print("         gather[%-7s] %d windows of %d bytes: median %.3f ms (min %.3f max %.3f) = %.2f TB/s read+written" % (
                shape, len(ms), 256 * 0xff00, float(np.median(ms)), min(ms), max(ms), 2 * 256 * 0xff00 / (float(np.median(ms)) * 1e-3) / 1e12), flush=True)
        print("         deflate per window median %.3f ms (min %.3f max %.3f); drain of %d windows %.2f s = %.2f GB/s of records" % (
            float(np.median(defl)), min(defl), max(defl), k, wall, info["total_bytes"] / wall / 1e9), flush=True)
        ims, iw = [], []
        for _ in range(5):   # thm_bam_sorter_index over the drained stream, repeated (the first call grows the pinned result)
            t0 = time.perf_counter(); bai, binfo = srt.index(1000); iw.append((time.perf_counter() - t0) * 1e3); ims.append(binfo["index_ms"])
        print("         index: %d bytes, %d bins, %d chunks, %d windows, %d records without a reference: index_ms median %.2f (min %.2f max %.2f), "
              "call median %.2f ms; sort_ms of this session %.2f" % (len(bai), binfo["n_bins"], binfo["n_chunks"], binfo["n_intervals"], binfo["n_no_coor"],
                                                                      float(np.median(ims)), min(ims), max(ims), float(np.median(iw)), sort_ms), flush=True)
        srt.close()
        b.close()
    if bgzf:
        import zlib
        K2 = 7
        names = [b"SYN:%d 1:N:0:ACGT" % i for i in range(n)]
        batch = dict(bases=bases, offsets=off, quals=np.full(len(bases), ord("F"), np.uint8), names=np.frombuffer(b"".join(names), np.uint8),
                     name_off=np.cumsum([0] + [len(x) for x in names]).astype("<u8"))

        def med(f):
            ms = []
            for _ in range(K2):
                t0 = time.perf_counter()
                r = f()
                ms.append((time.perf_counter() - t0) * 1e3)
            return r, float(np.median(ms)), min(ms), max(ms)

        b = capi.Aligner(ix, opts)
        b.upload_reads(batch)
        b.run(); b.sync()
        for _ in range(2):   # buffers grow
            b.fetch_bgzf(copy=False)
            b.fetch_bam(copy=False)
        tz = []
        for _ in range(K2):
            b.fetch_bgzf(copy=False)
            tz.append(b.timings()["bgzf"])
        # alternately, in one session
        mz, mg = [], []
        for _ in range(K2):
            t0 = time.perf_counter(); z = b.fetch_bgzf(copy=False); mz.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); g = b.fetch_bam(copy=False); mg.append((time.perf_counter() - t0) * 1e3)
        print("         fetch_bgzf  median %.2f ms (min %.2f max %.2f)  %d bytes to the host  %d blocks of %d raw bytes  THM_T_BGZF median %.3f ms (min %.3f max %.3f)" % (
            float(np.median(mz)), min(mz), max(mz), z.nbytes, z.n_blocks, z.n_raw_bytes, float(np.median(tz)), min(tz), max(tz)), flush=True)
        print("         fetch_bam   median %.2f ms (min %.2f max %.2f)  %d bytes to the host" % (float(np.median(mg)), min(mg), max(mg), g.nbytes), flush=True)
        raw = g.data.tobytes()
        dev_bytes = len(z.data)
        for threads in (16, 1):
            w = capi.Writer(ix, capi.FMT_BAM, n_threads=threads)
            w.wrap_bam(g)
            o, m, lo, hi = med(lambda: w.wrap_bam(g))
            print("         host, %2d threads: wrap_bam (deflate) median %.2f ms (min %.2f max %.2f); fetch_bam + wrap_bam = %.2f ms; %d bytes" % (
                threads, m, lo, hi, float(np.median(mg)) + m, len(o)), flush=True)
            w.close()
        z1 = 0
        for at in range(0, len(raw), 0xff00):
            c = zlib.compressobj(1, zlib.DEFLATED, -15)
            z1 += len(c.compress(raw[at: at + 0xff00]) + c.flush()) + 26
        print("         compressed sizes of %d record bytes: device %d, host encoder %d, zlib level 1 %d" % (len(raw), dev_bytes, len(o), z1), flush=True)
        b.close()
    if fastq:
        import os, tempfile
        K2 = 9
        reads = bases.reshape(n, 91)
        qual = b"F" * 91
        block = b"".join(b"@SYN:%d 1:N:0:ACGT\n" % i + reads[i].tobytes() + b"\n+\n" + qual + b"\n" for i in range(n))
        with tempfile.NamedTemporaryFile(suffix=".fastq", delete=False) as f:
            f.write(block)
        t0 = time.perf_counter()
        r = capi.FastqReader(f.name)
        batch = r.all_by_blocks(n)
        host_ms = (time.perf_counter() - t0) * 1e3   # (cut + parse + the copies of the test hook: an upper bound)
        r.close()
        os.remove(f.name)
        b = capi.Aligner(ix, opts)
        src = np.frombuffer(block, np.uint8)
        info = capi.FastqUploadInfo()
        rb, keep = capi.read_batch_struct(batch)

        def up_fastq():
            b._chk(capi.lib().thm_batch_upload_fastq(b.h, src.ctypes.data, len(block), b"perf", 1, 1, capi.C.byref(info)))

        def up_reads():
            b._chk(capi.lib().thm_batch_upload_reads(b.h, capi.C.byref(rb)))

        for _ in range(2):   # buffers grow
            up_fastq(); up_reads()
        mf, mr, md = [], [], []
        for _ in range(K2):   # alternately, in one session
            t0 = time.perf_counter(); up_fastq(); mf.append((time.perf_counter() - t0) * 1e3); md.append(info.device_ms)
            t0 = time.perf_counter(); up_reads(); mr.append((time.perf_counter() - t0) * 1e3)
        assert info.on_device == 1 and info.n_reads == n
        print("         upload_fastq median %.2f ms (min %.2f max %.2f)  block of %d bytes, %d reads  device_ms median %.3f (min %.3f max %.3f)" % (
            float(np.median(mf)), min(mf), max(mf), len(block), n, float(np.median(md)), min(md), max(md)), flush=True)
        print("         upload_reads median %.2f ms (min %.2f max %.2f)  %d bytes in five arrays; host cut + parse of the block, one thread, at most %.1f ms" % (
            float(np.median(mr)), min(mr), max(mr), sum(np.asarray(batch[k]).nbytes for k in batch), host_ms), flush=True)
        b.close()
    if fastq_bgzf:
        import struct, zlib
        K2 = 9
        reads = bases.reshape(n, 91)
        qual = b"F" * 91
        block = b"".join(b"@SYN:%d 1:N:0:ACGT\n" % i + reads[i].tobytes() + b"\n+\n" + qual + b"\n" for i in range(n))
        parts = []
        for at in range(0, len(block), 0xff00):
            piece = block[at: at + 0xff00]
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            z = c.compress(piece) + c.flush()
            parts.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(z) + 25) + z +
                         struct.pack("<II", zlib.crc32(piece), len(piece)))
        members = b"".join(parts)
        t0 = time.perf_counter()
        for m in parts:
            zlib.decompress(m, 31)
        zlib_ms = (time.perf_counter() - t0) * 1e3
        b = capi.Aligner(ix, opts)
        src, msrc = np.frombuffer(block, np.uint8), np.frombuffer(members, np.uint8)
        info, zinfo = capi.FastqUploadInfo(), capi.FastqBgzfInfo()

        def up_fastq():
            b._chk(capi.lib().thm_batch_upload_fastq(b.h, src.ctypes.data, len(block), b"perf", 1, 1, capi.C.byref(info)))

        def up_bgzf():
            b._chk(capi.lib().thm_batch_upload_fastq_bgzf(b.h, None, 0, msrc.ctypes.data, len(members), b"perf", 1, 1, capi.C.byref(zinfo)))

        for _ in range(2):   # buffers grow
            up_bgzf(); up_fastq()
        mz, mf, mi, mp = [], [], [], []
        for _ in range(K2):   # alternately, in one session
            t0 = time.perf_counter(); up_bgzf(); mz.append((time.perf_counter() - t0) * 1e3); mi.append(zinfo.inflate_ms); mp.append(zinfo.parse_ms)
            t0 = time.perf_counter(); up_fastq(); mf.append((time.perf_counter() - t0) * 1e3)
        assert zinfo.inflated_on_device == 1 and zinfo.parsed_on_device == 1 and zinfo.n_reads == n and info.n_reads == n
        print("         upload_fastq_bgzf median %.2f ms (min %.2f max %.2f)  %d members, %d -> %d bytes, %d reads  inflate_ms median %.3f (min %.3f max %.3f)  parse_ms median %.3f (min %.3f max %.3f)" % (
            float(np.median(mz)), min(mz), max(mz), len(parts), len(members), len(block), n, float(np.median(mi)), min(mi), max(mi),
            float(np.median(mp)), min(mp), max(mp)), flush=True)
        print("         upload_fastq of the inflated bytes median %.2f ms (min %.2f max %.2f); zlib inflate of the members, one host thread, %.1f ms" % (
            float(np.median(mf)), min(mf), max(mf), zlib_ms), flush=True)
        b.close()
    if fastq_gzip:
        import os, zlib
        K2 = 9
        reads = bases.reshape(n, 91)
        rng = np.random.default_rng(7)
        walk = np.clip(36 + np.cumsum(rng.integers(-2, 3, size=(n, 91)), axis=1), 2, 40).astype(np.uint8) + 33
        for label, qual_of in (("all-F qualities", lambda i: b"F" * 91), ("varied qualities", lambda i: walk[i].tobytes())):
            block = b"".join(b"@SYN:%d 1:N:0:ACGT\n" % i + reads[i].tobytes() + b"\n+\n" + qual_of(i) + b"\n" for i in range(n))
            c = zlib.compressobj(6, zlib.DEFLATED, 31)
            member = c.compress(block) + c.flush()
            t0 = time.perf_counter()
            assert len(zlib.decompress(member, 31)) == len(block)
            zlib_ms = (time.perf_counter() - t0) * 1e3
            b = capi.Aligner(ix, opts)
            src, msrc = np.frombuffer(block, np.uint8), np.frombuffer(member, np.uint8)
            info, zinfo = capi.FastqUploadInfo(), capi.FastqGzipInfo()

            def up_fastq():
                b._chk(capi.lib().thm_batch_upload_fastq(b.h, src.ctypes.data, len(block), b"perf", 1, 1, capi.C.byref(info)))

            def up_gzip():
                st = capi.GzipState()
                b._chk(capi.lib().thm_batch_upload_fastq_gzip(b.h, capi.C.byref(st), None, 0, msrc.ctypes.data, len(member), b"perf", 1, 1,
                                                              capi.C.byref(zinfo)))

            for _ in range(2):   # buffers grow
                up_gzip(); up_fastq()
            mz, mf, mi, mp = [], [], [], []
            for _ in range(K2):   # alternately, in one session
                t0 = time.perf_counter(); up_gzip(); mz.append((time.perf_counter() - t0) * 1e3); mi.append(zinfo.inflate_ms); mp.append(zinfo.parse_ms)
                t0 = time.perf_counter(); up_fastq(); mf.append((time.perf_counter() - t0) * 1e3)
            print("         %s, chunks of %s KiB: upload_fastq_gzip median %.2f ms (min %.2f max %.2f)  one member, %d -> %d bytes, %d reads  "
                  "inflated_on_device %d (decline_reason %d) n_chunks %d n_starts %d  inflate_ms median %.3f (min %.3f max %.3f)  "
                  "parse_ms median %.3f (min %.3f max %.3f)" % (
                      label, os.environ.get("THM_GZIP_CHUNK_KB", "32"), float(np.median(mz)), min(mz), max(mz), len(member), len(block), zinfo.n_reads,
                      zinfo.inflated_on_device, zinfo.decline_reason, zinfo.n_chunks, zinfo.n_starts, float(np.median(mi)), min(mi), max(mi),
                      float(np.median(mp)), min(mp), max(mp)), flush=True)
            print("         upload_fastq of the inflated bytes median %.2f ms (min %.2f max %.2f); zlib inflate of the member, one host thread, %.1f ms" % (
                float(np.median(mf)), min(mf), max(mf), zlib_ms), flush=True)
            assert zinfo.n_reads == n and info.n_reads == n
            if zinfo.inflated_on_device:
                _, _, counts = b.debug_gzip_inflate(capi.GzipState(), member, chunk_bytes=int(os.environ.get("THM_GZIP_CHUNK_KB", "32")) << 10, cap=len(block))
                print("         the device inflate alone: n_chunks %d n_starts %d starts the chain refused %d path flags %d" % counts, flush=True)
            b.close()
    c = dict(zip(capi.COUNTER_NAMES, a.counters().tolist()))
    runs = K + 2
    print("         per read: smems %.2f hits %.2f swg_calls %.2f cols %.1f cells %.0f alns %.2f win_bytes %.0f" % tuple(
        c[k] / (n * runs) for k in ("smems", "hits", "swg_calls", "dp_cols", "dp_cells", "alns", "window_bytes")), flush=True)
    if hasattr(a, "debug_tpr_stats"):
        es = a.debug_tpr_stats()
        names = {1: "band", 2: "grid", 3: "lift", 7: "other", 8: "rounds", 9: "candidates", 10: "edits", 11: "introns", 12: "pools", 13: "window", 14: "open"}
        print("         problem-parallel path: %d DP requests (narrow %d, by band class %s), %d reads left to the wave-per-read kernel (%s), "
              "%d still waiting after the last round" % (es[16], es[17], es[18:22].tolist(), es[0],
                                                         " ".join("%s %d" % (names.get(k, str(k)), es[k]) for k in range(1, 16) if es[k]), es[22]), flush=True)
    pr = a.debug_prof()
    if pr.sum() > 0:
        names = ["setup", "stage", "dp", "traceback", "tree", "txprep", "lift", "emit", "final", "other"]
        tot = float(pr[:10].sum())
        pc = lambda k: 100.0 * pr[k] / max(pr[10], 1)
        print("         DP columns: total %d, on <=32 slots %.1f%%, pairable (min of L/R when both <=32) %.1f%%, first hit of the read %.1f%%, "
              "transcript targets %.1f%%, one-mismatch-then-exact extensions %.1f%%" % (pr[10], pc(11), pc(12), pc(13), pc(14), pc(15)), flush=True)
        print("         extend sections: " + " ".join("%s=%.1f%%" % (nm, 100.0 * v / tot) for nm, v in zip(names, pr[:10])), flush=True)
    a.close()
