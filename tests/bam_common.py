"""Shared by tests/test_bam_host.py and tests/test_gpu_bam.py: the read sets the device BAM encoder is checked on, the
oracle's record stream for them, and a BAM record / aux parser written here from the SAM specification (section 4.2),
used to pin what the read sets contain and to remove tags."""
import os
import struct

import numpy as np

from gpu_common import MICRO_OPTS, beyond_team_reads, beyond_team_reference, micro_exon_reads, micro_exon_reference, ordinary_reads
from oracle import aln_writer as ow
from thermite_amd import capi, refdata, synth

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
GOLDEN_BIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_query.bam_records.bin")
GOLDEN_OPTS = dict(capi.DEFAULT_OPTS, min_seed_len=3, min_aln_score=0)  # the options of tests/golden/test_query.sam
ANNOTATION_TAGS = (b"TX", b"GX", b"GN", b"RE")
_ACGT = np.frombuffer(b"ACGT", np.uint8)


# ------------------------------------------------------------------ references (tables), by key
def tables(key):
    if key == "test_ref":
        return refdata.load_reference(DATA + "/test_ref.fasta", DATA + "/test_ref.gtf")
    if key == "chrm":
        return refdata.load_reference(DATA + "/GRCh38-2020-A-chrM.fasta", DATA + "/GRCh38-2020-A-chrM.gtf")
    if key == "syn":
        return synth.synth_reference(length=400000, n_genes=40)
    if key == "micro":
        return micro_exon_reference()
    if key == "multi":
        return multi_reference()
    if key == "beyond":
        t, info = beyond_team_reference()
        t["_info"] = info
        return t
    if key == "contigs":
        import contigs_common
        return contigs_common.world()[0]
    raise KeyError(key)


# ------------------------------------------------------------------ read sets
def _quals(rng, seqs):
    return [bytes(rng.integers(33, 74, len(s)).astype(np.uint8)) for s in seqs]


def _split(bases, off):
    return [bytes(bases[int(off[i]): int(off[i + 1])]) for i in range(len(off) - 1)]


def read_set(name, t):
    """-> dict(names, seqs, quals (None: a batch without qualities), opts); `t`: tables(REF_OF[name])"""
    rng = np.random.default_rng(sum(name.encode()))
    if name == "test_query":
        names, seqs, quals = refdata.parse_fastq(DATA + "/test_query.fastq")
        return dict(names=[n.encode() for n in names], seqs=[bytes(s) for s in seqs], quals=[bytes(q) for q in quals], opts=GOLDEN_OPTS)
    if name in ("chrm_ci", "chrm_default"):
        bases, off, _ = synth.simulate_reads(t, 3000, 91, sub_rate=0.02, indel_rate=0.004, stream=51, intronic_frac=0.25)
        seqs = _split(bases, off)
        return dict(names=[b"c%d" % i for i in range(len(seqs))], seqs=seqs, quals=_quals(rng, seqs),
                    opts=capi.CI_OPTS if name == "chrm_ci" else capi.DEFAULT_OPTS)
    if name == "syn":
        # spliced, intronic and intergenic reads of a multi-exon reference; reads from its repeat families (multi-mapped);
        # random reads (unmapped); even and odd lengths; lowercase and N bases; names with a comment behind a space
        bases, off, _ = synth.simulate_reads(t, 4000, 91, sub_rate=0.02, indel_rate=0.004, stream=41, intronic_frac=0.2)
        seqs = _split(bases, off)
        b2, o2, _ = synth.simulate_reads(t, 600, 90, sub_rate=0.01, indel_rate=0.002, stream=42, intronic_frac=0.3)
        seqs += _split(b2, o2)
        for i in range(0, len(seqs), 9):
            seqs[i] = bytes(_ACGT[rng.integers(0, 4, 91 - (i % 2))])
        for i in range(1, len(seqs), 7):   # lowercase stretches, and an N
            s = bytearray(seqs[i])
            lo = int(rng.integers(0, len(s) - 20))
            s[lo: lo + 15] = bytes(s[lo: lo + 15]).lower()
            if i % 2:
                s[int(rng.integers(0, len(s)))] = ord("N")
            seqs[i] = bytes(s)
        names = [(b"r%d 1:N:0:ACGT" % i) if i % 3 else (b"r%d" % i) for i in range(len(seqs))]
        return dict(names=names, seqs=seqs, quals=_quals(rng, seqs), opts=capi.CI_OPTS)
    if name == "micro":   # alignments along transcripts of hundreds of 1-base exons; no qualities (FASTA input)
        bases, off, _ = micro_exon_reads(t, lengths=(91, 250), stride=13)
        seqs = _split(bases, off)
        return dict(names=[b"m%d" % i for i in range(len(seqs))], seqs=seqs, quals=None, opts=MICRO_OPTS)
    if name == "multi":   # reads with exactly 2, 3, 4 and 7 places, both orientations, among ordinary ones
        seqs = []
        for k, u in enumerate(t["_units"]):
            seqs += [bytes(u), bytes(refdata.revcomp(u))]
        bases, off, _ = synth.simulate_reads(t, 200, 91, sub_rate=0.01, indel_rate=0.001, stream=43)
        seqs += _split(bases, off)
        return dict(names=[b"u%d" % i for i in range(len(seqs))], seqs=seqs, quals=_quals(rng, seqs), opts=capi.CI_OPTS)
    if name == "beyond":  # reads with 60 000 and 60 001 seed hits, hundreds of tying places
        reads, kinds = beyond_team_reads(t["_info"], np.random.default_rng(2))
        ob, oo = ordinary_reads(t, 300, stream=2)
        seqs = [bytes(r) for r in reads] + _split(ob, oo)
        order = rng.permutation(len(seqs))
        seqs = [seqs[i] for i in order]
        return dict(names=[b"b%d" % i for i in range(len(seqs))], seqs=seqs, quals=_quals(rng, seqs),
                    opts=dict(capi.CI_OPTS, multimap_score_range=6))
    if name == "contigs":  # many contigs, names not in byte order: alignments of one read on several references, most references short
        import contigs_common
        seqs = contigs_common.read_set()["seqs"]
        return dict(names=[b"g%d" % i for i in range(len(seqs))], seqs=seqs, quals=_quals(rng, seqs), opts=capi.CI_OPTS)
    raise KeyError(name)


MULTI_COPIES = (2, 3, 4, 7)


def multi_reference(seed=0x62616D):
    """A random contig with ordinary genes in its first part and, behind them, four 91-mers planted 2, 3, 4 and 7 times:
    a read that is one of them has that many equally good places (NH 2, 3, 4 and >= 5: the whole MAPQ table)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gene_region, length = 60000, 72000
    seq = _ACGT[rng.integers(0, 4, length)]
    units = [_ACGT[rng.integers(0, 4, 91)] for _ in MULTI_COPIES]
    p = gene_region + 300
    for u, c in zip(units, MULTI_COPIES):
        for _ in range(c):
            seq[p: p + 91] = u
            p += 91 + int(rng.integers(150, 400))
    assert p < length - 200
    genes, txs = synth.synth_annotation(rng, "multisyn", gene_region, 500, 6)
    t = refdata.build_tables([("multisyn", seq)], genes, txs)
    t["_units"] = units
    return t


REF_OF = dict(test_query="test_ref", chrm_ci="chrm", chrm_default="chrm", syn="syn", multi="multi", micro="micro", beyond="beyond",
              contigs="contigs")
READ_SETS = list(REF_OF)


def batch_of(rs):
    """the dict capi.Aligner.upload_reads / FastqReader.next_batch use"""
    seqs, names = rs["seqs"], rs["names"]
    return dict(bases=np.frombuffer(b"".join(seqs), np.uint8), offsets=np.cumsum([0] + [len(s) for s in seqs]).astype("<u8"),
                quals=None if rs["quals"] is None else np.frombuffer(b"".join(rs["quals"]), np.uint8),
                names=np.frombuffer(b"".join(names), np.uint8), name_off=np.cumsum([0] + [len(n) for n in names]).astype("<u8"))


def oracle_records(t, rs, result):
    """the oracle's record stream for the read set (header removed) and the byte offset of every read's first record"""
    quals = rs["quals"] if rs["quals"] is not None else [b""] * len(rs["seqs"])
    stream = ow.bam_stream(t, rs["names"], rs["seqs"], quals, result)
    hdr = ow.bam_header_bytes(t)
    assert stream[: len(hdr)] == hdr
    data = stream[len(hdr):]
    n_rec = np.maximum(np.diff(result.offsets.astype(np.int64)), 1)
    off, at = [0], 0
    for k in n_rec:
        for _ in range(int(k)):
            at += 4 + struct.unpack_from("<I", data, at)[0]
        off.append(at)
    assert at == len(data)
    return data, np.array(off, "<u8")


# ------------------------------------------------------------------ BAM records, SAM specification section 4.2
_AUX_SIZE = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}


def parse_aux(b):
    """[(tag, type, raw value bytes, whole field bytes)] of the aux region of one record"""
    out, at = [], 0
    while at < len(b):
        tag, ty = b[at: at + 2], b[at + 2: at + 3]
        if ty in _AUX_SIZE:
            n = _AUX_SIZE[ty]
        elif ty in (b"Z", b"H"):
            n = b.index(b"\0", at + 3) - (at + 3) + 1
        elif ty == b"B":
            sub = b[at + 3: at + 4]
            n = 5 + _AUX_SIZE[sub] * struct.unpack_from("<I", b, at + 4)[0]
        else:
            raise ValueError("aux type %r" % ty)
        out.append((tag, ty, b[at + 3: at + 3 + n], b[at: at + 3 + n]))
        at += 3 + n
    return out


def parse_record(rec):
    """one record (with its block_size) -> dict"""
    bs, = struct.unpack_from("<I", rec, 0)
    assert bs + 4 == len(rec)
    ref_id, pos, l_name, mapq, bin_, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 4)
    at = 36
    qname = rec[at: at + l_name - 1]
    assert rec[at + l_name - 1] == 0
    at += l_name
    cigar = struct.unpack_from("<%dI" % n_cig, rec, at)
    at += 4 * n_cig
    seq = rec[at: at + (l_seq + 1) // 2]
    at += (l_seq + 1) // 2
    qual = rec[at: at + l_seq]
    at += l_seq
    return dict(ref_id=ref_id, pos=pos, mapq=mapq, bin=bin_, flag=flag, l_seq=l_seq, qname=qname, cigar=cigar, seq=seq, qual=qual,
                aux_at=at, aux=parse_aux(rec[at:]))


def split_records(data):
    data = bytes(data)
    out, at = [], 0
    while at < len(data):
        n = 4 + struct.unpack_from("<I", data, at)[0]
        out.append(data[at: at + n])
        at += n
    assert at == len(data)
    return out


def strip_annotation(data):
    """the record stream with TX GX GN RE removed from every record (block_size adjusted) -- record.remove_aux,
    src/wrapper.rs:136-139"""
    out = []
    for rec in split_records(data):
        r = parse_record(rec)
        body = rec[4: r["aux_at"]] + b"".join(f for tag, _, _, f in r["aux"] if tag not in ANNOTATION_TAGS)
        out.append(struct.pack("<I", len(body)) + body)
    return b"".join(out)
