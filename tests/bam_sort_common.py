"""Shared by tests/test_bam_sort_host.py and tests/test_gpu_bam_sort.py: synthetic BAM records, the expectation for the
coordinate sort (written here from the order include/thermite_io.h states: split, key, numpy's stable argsort, join) and
the oracle's BAM header with the @HD line of a sorted file.  Nothing here comes from the code under test."""
import struct

import numpy as np

import bam_common as bc
from oracle import aln_writer as ow

BLOCK_IN = 0xff00
HD_LINE = b"@HD\tVN:1.6\tSO:coordinate\n"
POS_MAX = 2 ** 31 - 2


def make_record(ref_id, pos, flag, name=b"r", l_seq=0):
    """a well-formed record without CIGAR or aux: block_size, the fixed fields, the name, l_seq bases and qualities"""
    name = bytes(name) + b"\0"
    seq = bytes((17 * (i + l_seq)) & 0xff for i in range((l_seq + 1) // 2))
    qual = bytes((i * 7 + pos) & 0x3f for i in range(l_seq))
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name), 0, 4680, 0, flag, l_seq, -1, -1, 0) + name + seq + qual
    return struct.pack("<I", len(body)) + body


def keys_of(records, n_sq):
    out = np.zeros(len(records), np.uint64)
    for i, rec in enumerate(records):
        ref_id, pos = struct.unpack_from("<ii", rec, 4)
        flag, = struct.unpack_from("<H", rec, 18)
        rank = ref_id if ref_id >= 0 else n_sq
        out[i] = (rank << 33) | (((pos + 1) & 0xffffffff) << 1) | ((flag >> 4) & 1)
    return out


def sorted_stream(data, n_sq):
    """the record stream `data` in coordinate order, ties in input order"""
    records = bc.split_records(data)
    order = np.argsort(keys_of(records, n_sq), kind="stable")
    return b"".join(records[i] for i in order)


def n_sq_of(t):
    """number of reference sequences in the oracle's BAM header"""
    hdr = ow.bam_header_bytes(t)
    l_text, = struct.unpack_from("<I", hdr, 4)
    return struct.unpack_from("<I", hdr, 8 + l_text)[0]


def sorted_header_bytes(t):
    """oracle.aln_writer.bam_header_bytes(t) with the @HD line in front of the text (l_text adjusted)"""
    hdr = ow.bam_header_bytes(t)
    assert hdr[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<I", hdr, 4)
    return hdr[:4] + struct.pack("<I", l_text + len(HD_LINE)) + HD_LINE + hdr[8:]


def windows_of(stream, window):
    return [stream[at: at + window] for at in range(0, len(stream), window)]


def synthetic_cases(n_sq=4):
    """name -> record stream: the edge cases of the order and of the window cuts"""
    rng = np.random.default_rng(0x50f7)
    cases = {"empty": b""}
    # thousands of records with one key among a few others: only stability orders them
    recs = [make_record(1, 500, 0, b"t%d" % i, l_seq=int(rng.integers(0, 9))) for i in range(3000)]
    recs[100] = make_record(0, 7, 16, b"early")
    recs[2000] = make_record(-1, -1, 4, b"unmapped")
    recs[2500] = make_record(1, 500, 16, b"reverse")
    cases["ties"] = b"".join(recs)
    # the ends of the position range, both strands, every rank including the unmapped one
    recs = []
    for ref_id in list(range(n_sq)) + [-1]:
        for pos in (-1, 0, 1, POS_MAX - 1, POS_MAX):
            for flag in (0, 16, 4 if ref_id < 0 else 256):
                recs.append(make_record(ref_id, pos, flag, b"p%d_%d_%d" % (ref_id + 1, pos & 0xffff, flag), l_seq=5))
    recs = [recs[i] for i in rng.permutation(len(recs))]
    cases["positions"] = b"".join(recs)
    # a record longer than a whole window of one block, among small ones
    recs = [make_record(int(rng.integers(-1, n_sq)), int(rng.integers(0, 1000)), int(rng.integers(0, 2)) * 16, b"s%d" % i, l_seq=int(rng.integers(0, 60)))
            for i in range(400)]
    # one in the middle of the sorted stream (it straddles window boundaries at both ends) and one that sorts first and so
    # covers the whole first window
    recs.insert(123, make_record(2, 400, 0, b"long", l_seq=46000))
    recs.insert(300, make_record(0, -1, 0, b"long_first", l_seq=46000))
    cases["long_record"] = b"".join(recs)
    assert len(recs[123]) > BLOCK_IN + 3000
    return cases
