"""The figures DESIGN.md section 4.21 quotes for thm_cells, on one device.

    python tools/cells_measure.py [ref_len=4000000] [n_batches=16] [e2e_reads=2000000] [rounds=3]

1. n_batches distinct batches of 500 000 reads of 91 bases (tools/e2e.py's reference and read model, streams 7, 8, ...),
   each with names "S<7 digits>_<barcode>_<UMI>": barcodes from a pool of 5 000, UMIs at random, so nearly every counted
   read is a molecule of its own and the table grows with every batch.  Every batch goes through thm_cells_add and, beside
   it, thm_quant_add: add_ms of both, n_molecules and n_pending behind every add (an add with n_pending 0 merged).
   Then fetch_ms at min_umis 1 and 100, three times each, and the first batch added five more times.
2. A FASTQ file of e2e_reads such reads to BAM with THM_BAM_DEVICE=1 through thm_align_files, without and with
   THM_CELLS=1 alternately, `rounds` rounds: the file-to-file rate."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thermite_amd import capi, synth  # noqa: E402

ref_len = int(sys.argv[1]) if len(sys.argv) > 1 else 4000000
n_batches = int(sys.argv[2]) if len(sys.argv) > 2 else 16
e2e_reads = int(sys.argv[3]) if len(sys.argv) > 3 else 2000000
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
N, L = 500000, 91
ACGT = np.frombuffer(b"ACGT", np.uint8)
rng = np.random.default_rng(5000)
POOL = ACGT[rng.integers(0, 4, (5000, 16))]


def names_of(n, first):
    """n names of 38 bytes as an (n, 38) array: S, seven digits, _, barcode, _, UMI"""
    out = np.empty((n, 38), np.uint8)
    out[:, 0] = ord("S")
    idx = (first + np.arange(n)) % 10000000
    for d in range(7):
        out[:, 7 - d] = ord("0") + idx % 10
        idx //= 10
    out[:, 8] = out[:, 25] = ord("_")
    out[:, 9:25] = POOL[rng.integers(0, len(POOL), n)]
    out[:, 26:38] = ACGT[rng.integers(0, 4, (n, 12))]
    return out


t = synth.synth_reference(length=ref_len)
ix = capi.Index(t)
a = capi.Aligner(ix, capi.CI_OPTS)
c, q = capi.Cells(a), capi.Quant(a)
first_batch = None
for k in range(n_batches):
    b, o, _ = synth.simulate_reads(t, N, L, sub_rate=0.01, indel_rate=0.001, stream=7 + k)
    nm = names_of(N, k * N)
    batch = dict(bases=b, offsets=o, quals=None, names=nm.reshape(-1), name_off=(np.arange(N + 1, dtype="<u8") * 38))
    first_batch = first_batch or batch
    a.upload_reads(batch)
    a.run()
    ci = c.add()
    qi = q.add()
    print("batch %2d: cells add_ms %.3f | counted %d untagged %d multi %d | n_molecules %d n_pending %d held %.1f MB | quant add_ms %.3f" % (
        k + 1, ci["add_ms"], ci["n_counted_reads"], ci["n_untagged_reads"], ci["n_multi_reads"], ci["n_molecules"], ci["n_pending"],
        ci["held_bytes"] / 1e6, qi["add_ms"]), flush=True)
for m in (1, 100):
    f = [c.fetch(m) for _ in range(3)]
    print("fetch min_umis %d: fetch_ms %s | %d molecules, %d barcodes, %d cells, %d entries" % (
        m, " ".join("%.3f" % x.fetch_ms for x in f), f[0].n_molecules, f[0].n_barcodes, len(f[0].cells), len(f[0].entries)), flush=True)
a.upload_reads(first_batch)
a.run()
again = [c.add() for _ in range(5)]
print("the first batch five more times (every molecule is in the table): cells add_ms %s | n_pending %s | quant add_ms %s" % (
    " ".join("%.3f" % x["add_ms"] for x in again), " ".join(str(x["n_pending"]) for x in again), " ".join("%.3f" % q.add()["add_ms"] for _ in range(5))),
    flush=True)
c.close()
q.close()

# ---- file to file
if e2e_reads:
    b, o, _ = synth.simulate_reads(t, e2e_reads, L, sub_rate=0.01, indel_rate=0.001, stream=100)
    rec = np.empty((e2e_reads, 1 + 38 + 1 + L + 3 + L + 1), np.uint8)
    rec[:, 0] = ord("@")
    rec[:, 1:39] = names_of(e2e_reads, 0)
    rec[:, 39] = rec[:, 40 + L] = rec[:, 42 + L] = rec[:, -1] = ord("\n")
    rec[:, 40:40 + L] = b.reshape(e2e_reads, L)
    rec[:, 41 + L] = ord("+")
    rec[:, 43 + L:43 + 2 * L] = ord("F")
    path, out = "/tmp/thm_cells_measure.fastq", "/tmp/thm_cells_measure_out.bam"
    rec.tofile(path)
    print("fastq: %d reads, %.1f MB" % (e2e_reads, os.path.getsize(path) / 1e6), flush=True)
    os.environ["THM_BAM_DEVICE"] = "1"
    for k in range(rounds):
        for tag, knob in (("plain", None), ("cells", "1")):
            os.environ.pop("THM_CELLS", None)
            if knob:
                os.environ["THM_CELLS"] = knob
            t0 = time.time()
            st = capi.align_files(a, [path], out, capi.FMT_BAM)
            side = ""
            if knob:
                side = ", cells.mtx %d bytes" % os.path.getsize(out + ".cells.mtx")
                for s in (".cells.mtx", ".cells.barcodes.tsv", ".cells.features.tsv"):
                    os.remove(out + s)
            print("bam %s round %d: %.2f Mreads/s wall %.3fs (%.3fs with the call) | parse %.2fs gpu %.2fs format %.2fs write %.2fs | %d batches%s" % (
                tag, k, st["n_reads"] / st["wall_s"] / 1e6, st["wall_s"], time.time() - t0, st["parse_s"], st["gpu_s"], st["format_s"], st["write_s"],
                st["n_batches"], side), flush=True)
    os.environ.pop("THM_CELLS", None)
    os.remove(out)
    os.remove(path)
a.close()
