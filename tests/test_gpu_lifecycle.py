"""-m gpu: an aligner and its index give back the device memory they took (free device memory is what the test reads:
pinned memory, events and streams do not show in it).  The device buffers of thm_aligner and of the index's device copy
free themselves (aligner_internal.h); a stage whose buffers were never freed would lose the aligner's footprint once per
create / close cycle.  Each cycle runs every stage once -- the four fetches with a read
beyond MAX_READ_LEN among the reads, so that the statuses travel; the FASTQ parser; the per-hit and the seed-only entry
points -- and each cycle's results are those of the first, byte for byte."""
import numpy as np
import pytest
import torch

import bam_common as bc
from thermite_amd import capi, synth

pytestmark = pytest.mark.gpu

N_READS, READ_LEN, LONG_AT = 2000, 120, 1234


def _inputs():
    t = synth.synth_reference(length=300000, n_genes=30)
    bases, off, _ = synth.simulate_reads(t, N_READS, READ_LEN, sub_rate=0.02, indel_rate=0.004, stream=61)
    seqs = [bytes(bases[int(off[i]): int(off[i + 1])]) for i in range(N_READS)]
    with_long = list(seqs)
    with_long.insert(LONG_AT, b"ACGT" * 17000)  # 68 000 bases: beyond MAX_READ_LEN
    names = [b"r%d" % i for i in range(len(with_long))]
    quals = [b"I" * len(s) for s in with_long]
    batch = bc.batch_of(dict(names=names, seqs=with_long, quals=quals))
    fastq = b"".join(b"@%s\n%s\n+\n%s\n" % r for r in zip(names, with_long, quals))
    return t, batch, fastq, (bases, off)


def _free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def _cycle(t, batch, fastq, short):
    """-> (every result as bytes, the aligner's footprint: free device memory after its close() minus before)"""
    ix = capi.Index(t)
    a = capi.Aligner(ix, capi.CI_OPTS)
    out = []

    def keep(*arrays):
        out.extend(None if x is None else np.ascontiguousarray(x).tobytes() for x in arrays)

    g = a.align_batch(batch["bases"], batch["offsets"])
    assert g.n_failed == 1 and g.status[LONG_AT] == capi.ERR_UNSUPPORTED and len(g.alns) > N_READS // 2
    keep(g.offsets, g.alns, g.ops, g.status)
    c = a.align_batch_cigars(batch["bases"], batch["offsets"])
    keep(c.offsets, c.alns, c.digests, c.cigar, c.status)
    b = a.align_batch_bam(batch)
    keep(b.data, b.read_rec_off, b.status)
    z = a.align_batch_bgzf(batch)
    keep(z.data, z.block_off, z.status)
    assert c.n_failed == b.n_failed == z.n_failed == 1
    info = a.upload_fastq(fastq)
    assert info["on_device"] == 1 and info["n_reads"] == N_READS + 1
    r = a.fetch_reads()
    keep(r["bases"], r["offsets"], r["quals"], r["names"], r["name_off"])
    hit_off, hits = a.smems_batch(short[0], short[1], 20)
    keep(hit_off, hits)
    assert len(hits) > N_READS // 2
    bw = np.full(len(hits), 40, "<u4")
    keep(*a.align_seed_hits(short[0], short[1], hit_off, hits, bw, bw.astype("<i4"), 40))
    before = _free()
    a.close()
    footprint = _free() - before
    ix.close()
    return out, footprint


def test_create_run_close_cycles_return_their_memory():
    torch.cuda.init()
    inputs = _inputs()
    first, _ = _cycle(*inputs)  # warm-up: code objects, the runtime's own pools
    f1 = _free()
    footprint = None
    for k in range(4):
        got, p = _cycle(*inputs)
        footprint = p if footprint is None else footprint
        assert got == first, "cycle %d differs from the first" % (k + 2)
    f5 = _free()
    print("free after the warm-up cycle %d, after four more %d, lost %d; the aligner's footprint %d" % (f1, f5, f1 - f5, footprint))
    assert footprint > 0, "closing the aligner returned nothing: the condition below would mean nothing"
    # a stage whose buffers are never freed would cost about 4 * footprint
    assert f1 - f5 < footprint / 2
