"""Shared by tests/test_fastq_device_host.py and tests/test_gpu_fastq_device.py: the blocks the device FASTQ parser
(thermite_amd/csrc/fastq_device.h, kernels_fastq.hip, thm_batch_upload_fastq) is checked on, and the host parser's
outcome for them -- capi.FastqReader(...).all_by_blocks, i.e. fastq_parse_block -- which is the reference throughout.

well_formed(): blocks in the strict form; the device must take every one.
declined(): blocks the device must hand to the host parser, whose batch or ERR_FORMAT message is then the outcome."""
import os

import numpy as np

from thermite_amd import capi

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
CHUNK = 4096   # fq::CHUNK of fastq_device.h: bytes per newline count, one wave's walk
STEP = 256     # fq::STEP: bytes a wave takes at a time
KEYS = ("names", "name_off", "bases", "offsets", "quals")
LONG_READ = 200000   # beyond the 65535 bases a read may have: parsed, then THM_ERR_UNSUPPORTED for that read
_ALPHABET = np.frombuffer(b"ACGTNacgt", np.uint8)


def _record(rng, name, L):
    seq = bytes(_ALPHABET[rng.integers(0, 9, L)])
    qual = bytes(rng.integers(33, 74, L).astype(np.uint8))   # '@' (64) and '+' (43) occur, also first in the line
    return b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n"


def random_records(n=533, seed=5):
    """the records of test_fastq_block_parser_equals_sequential_parser (tests/test_io_host.py): lengths 0..159, names
    with spaces; the first two quality lines begin with '@' and '+'"""
    rng = np.random.default_rng(seed)
    recs = [_record(rng, b"r%d some words %d" % (i, i * 7), int(rng.integers(0, 160))) for i in range(n)]
    for i, c in ((0, b"@"), (1, b"+")):
        name, seq, plus, qual = recs[i].split(b"\n")[:4]
        if not seq:
            seq, qual = b"ACGT", b"IIII"
        recs[i] = name + b"\n" + seq + b"\n+\n" + c + qual[1:] + b"\n"
    return recs


def well_formed():
    rng = np.random.default_rng(11)
    recs = random_records()
    plain = b"".join(recs)
    out = {"random": plain, "crlf": plain.replace(b"\n", b"\r\n"), "no_final_newline": plain[:-1],
           "cr_cr_lf": b"".join(recs[:40]).replace(b"\n", b"\r\r\n"), "one_record": b"@only one\nACGTN\n+\n!!!!#\n",
           "one_record_no_newline": b"@x\nA\n+\nI"}
    # read lengths either side of the 64 bytes a wave's lanes number and of twice that
    out["lengths_62_66_126_130"] = b"".join(_record(rng, b"s%d" % L, L) for L in (62, 63, 64, 65, 66, 126, 127, 128, 129, 130) * 3)
    # exactly two chunks: the last name is padded to the byte
    body = b"".join(recs[:20])
    assert len(body) < 2 * CHUNK - 64
    tail = _record(rng, b"t", 10)
    pad = 2 * CHUNK - len(body) - len(tail)
    out["two_chunks_exactly"] = body + tail.replace(b"@t", b"@t" + b"x" * pad, 1)
    assert len(out["two_chunks_exactly"]) == 2 * CHUNK and out["two_chunks_exactly"].endswith(b"\n")
    # the header's newline is the last byte of the first chunk, the (empty) sequence line's the first of the second
    body = b"".join(recs[2:12])
    assert len(body) < CHUNK - 64
    blk = body + b"@e" + b"y" * (CHUNK - 1 - len(body) - 2) + b"\n" + b"\n+\n\n" + b"".join(recs[12:20])
    assert blk[CHUNK - 1: CHUNK + 1] == b"\n\n"
    out["newline_either_side_of_a_chunk"] = blk
    out["empty_read_in_the_middle"] = b"".join(recs[:5]) + b"@empty read\n\n+\n\n" + b"".join(recs[5:9])
    out["long_read"] = b"".join(recs[20:27]) + _record(rng, b"long one", LONG_READ) + b"".join(recs[27:31])
    out["test_query"] = open(os.path.join(DATA, "test_query.fastq"), "rb").read()
    return out


LONG_READ_INDEX = 7   # of the long read in well_formed()["long_read"]


def declined():
    """name -> (block, last_block, the file whose one-block parse is the reference).  For a block that is not the last of
    its input the reference file is the block with one more record behind it: the host parser meets the same line at the
    same number, with input behind it."""
    recs = random_records(12, seed=6)
    body = b"".join(recs)
    more = b"@more\nA\n+\nI\n"
    out = {"blank_tail_last": (body + b"\n\n", True, body + b"\n\n"),
           "blank_tail_not_last": (body + b"\n\n", False, body + b"\n\n" + more),
           "blank_line_between": (b"@a\nAC\n+\n!!\n\n@b\nAC\n+\n!!\n", True, None),
           "quality_one_short_of_9000": (b"@r0\n" + b"A" * 9000 + b"\n+\n" + b"I" * 8999 + b"\n", True, None),
           "empty_read_without_quality_line": (body + b"@n\n\n+\n", True, None),
           "header_only_cr": (body + b"\r\nACGT\n+\nIIII\n", True, None),
           "four_blank_lines_last": (body + b"\n\n\n\n", True, None)}
    for k, bad in enumerate((b"@r\nACGT\n+\n!!\n", b"@r\nACGT\nACGT\n!!!!\n", b"ACGT\n", b"@r\nACGT\n")):   # test_fastq_batcher_edge_cases
        out["bad_%d" % k] = (bad, True, None)
    out["bad_1_after_records"] = (body + b"@r\nACGT\nACGT\n!!!!\n", True, None)
    out["bad_2_after_records"] = (body + b"ACGT\n", True, None)
    out["bad_2_four_lines"] = (b"ACGT\nAC\n+\n!!\n", True, None)   # a leading non-'@' with the line count in order
    return {k: (blk, last, blk if ref is None else ref) for k, (blk, last, ref) in out.items()}


def host_parse(path):
    """fastq_parse_block over the file as one block (the last of its input) -> the batch dict; ThermiteError as it raises"""
    r = capi.FastqReader(path)
    try:
        return r.all_by_blocks(1 << 40)
    finally:
        r.close()


def host_outcome(tmp_path, name, data):
    """('batch', dict) or ('error', code, message) of the host parser for the bytes, as the file tmp_path/name.fastq;
    an empty batch for a file the block cutter finds nothing in"""
    p = tmp_path / (name + ".fastq")
    p.write_bytes(data)
    try:
        return ("batch", host_parse(p)), str(p)
    except capi.ThermiteError as e:
        if not data.startswith(b"@"):
            # all_by_blocks turns such a file away before it cuts a block ("not a plain FASTQ input"; the file driver
            # gives it to the sequential parser).  The block parser, which is what stands behind thm_batch_upload_fastq,
            # reports the first line in its own words: the code is all_by_blocks', the message is spelled out here.
            assert e.code == capi.ERR_FORMAT
            return ("error", e.code, "expected '@' at %s:1" % p), str(p)
        return ("error", e.code, message(e)), str(p)


def message(e):
    """a ThermiteError's message without the code in front of it"""
    return str(e).split(": ", 1)[1]


def batches_differ(got, want):
    """the first of the five arrays that differs, or None"""
    for k in KEYS:
        g, w = got[k], want[k]
        if g is None or w is None:
            if not (g is None and w is None):
                return k
        elif not np.array_equal(np.asarray(g), np.asarray(w)):
            return k
    return None


def fastq_text(rs, eol=b"\n"):
    """a read set of bam_common (names, seqs, quals) as FASTQ text"""
    return b"".join(b"@" + n + eol + s + eol + b"+" + eol + q + eol for n, s, q in zip(rs["names"], rs["seqs"], rs["quals"]))
