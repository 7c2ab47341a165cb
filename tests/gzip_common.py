"""Shared by tests/test_gzip_device_host.py and tests/test_gpu_gzip_device.py: the gzip streams the device inflater for
plain gzip (thermite_amd/csrc/gzip_device.h, kernels_gzip.hip, thm_batch_upload_fastq_gzip) is checked on, and the
runner of its host model (tests/cpp/gzip_model_main.cpp).  Everything is built here with zlib and the bit writer of
inflate_common; nothing is committed as binary.  The reference for the bytes is gzip.decompress; for consumption, states
and errors it is the host path, GzInflater's resume entry (capi.debug_gzip_host_slice).

well_formed():  name -> Fixture: streams the device must inflate at every chunk size (no decline is allowed)
declined():     valid gzip built to be declined, and the status it is declined with: the host inflater's bytes are the result
corrupt():      name -> (stream, statuses the model may end with): then the host inflater's ERR_IO"""
import collections
import functools
import os
import random
import struct
import subprocess
import zlib

import inflate_common as ic
from thermite_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Fixture = collections.namedtuple("Fixture", "stream data fastq")   # fastq: the inflated bytes are whole FASTQ records
# status words and path flags of gzip_device.h (the first twelve are inflate_device.h's)
OK, TRUNCATED, BLOCK_TYPE, STORED_LEN, CODE_LENGTHS, BAD_CODE, DISTANCE, OUTPUT, CRC, TABLE_ROOM, TRAILING, MEMBER = range(12)
NO_MEET, REACH, REGION, MEMBER_CAP, HEADER, ISIZE, INPUT = range(12, 19)
G_MARKER, G_MARKER_COPY, G_MERGED, G_WIN_IN_WIN, G_MEMBER_END, G_ROLLBACK, G_REACH = 1, 2, 4, 8, 16, 32, 64
FLAG_NAMES = {G_MARKER: "marker", G_MARKER_COPY: "marker copied from a run's own output", G_MERGED: "start-less chunk merged into a run",
              G_WIN_IN_WIN: "window reaching into the predecessor's window", G_MEMBER_END: "member end inside a run",
              G_ROLLBACK: "rollback of the last run", G_REACH: "reach check"}
DEFAULT_CHUNK = 32768
MODEL_CHUNKS = (64, 256, 1024, 4096, DEFAULT_CHUNK)
MODEL_SLICES = (7000, 20000, 0)      # 0: the whole stream in one call
GPU_CHUNKS = (256, 4096, DEFAULT_CHUNK)
SEED = 20261019


@functools.lru_cache(maxsize=None)
def text(n_reads=2000, seed=SEED):
    """FASTQ of n_reads reads of 91 bases, names and qualities varied"""
    rnd = random.Random(seed)
    out = []
    for i in range(n_reads):
        name = "@M%05d:%d:FC%s:%d:%d:%d %d:N:0:%s" % (rnd.randrange(99999), rnd.randrange(300), "".join(rnd.choice("ABCDXY") for _ in range(5)),
                                                  rnd.randrange(1, 9), rnd.randrange(1000, 30000), rnd.randrange(1000, 30000), 1 + i % 2,
                                                  "".join(rnd.choice("ACGT") for _ in range(rnd.randrange(0, 9))))
        seq = "".join(rnd.choice("ACGT") if rnd.random() > 0.002 else "N" for _ in range(91))
        q, qual = 36, []
        for _ in range(91):
            q = min(40, max(2, q + rnd.choice((-3, -1, 0, 0, 0, 0, 1, 2))))
            qual.append(chr(33 + q))
        out.append("%s\n%s\n+\n%s\n" % (name, seq, "".join(qual)))
    return "".join(out).encode()


def small():
    return text(14)


def header(fextra=None, fname=None, fcomment=None, fhcrc=False):
    flg = (4 if fextra is not None else 0) | (8 if fname is not None else 0) | (16 if fcomment is not None else 0) | (2 if fhcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff"
    if fextra is not None:
        h += struct.pack("<H", len(fextra)) + fextra
    if fname is not None:
        h += fname + b"\0"
    if fcomment is not None:
        h += fcomment + b"\0"
    if fhcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h


def frame(payload, data, crc=None, isize=None, **hdr):
    """a raw DEFLATE stream as a gzip member"""
    return header(**hdr) + payload + struct.pack("<II", zlib.crc32(data) if crc is None else crc, (len(data) if isize is None else isize) & 0xFFFFFFFF)


def raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return c.compress(data) + c.flush()


def member(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, **hdr):
    return frame(raw(data, level, strategy, mem_level), data, **hdr)


def _flushed(data):
    """a Z_SYNC_FLUSH every 2 KB and one Z_FULL_FLUSH"""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    out = []
    for k, i in enumerate(range(0, len(data), 2048)):
        out.append(c.compress(data[i: i + 2048]))
        out.append(c.flush(zlib.Z_FULL_FLUSH if k == 7 else zlib.Z_SYNC_FLUSH))
    return b"".join(out) + c.flush()


def _noise(n, seed):
    """literals of a 16-letter alphabet: 4 bits each in a dynamic block"""
    rnd = random.Random(seed)
    return [rnd.choice(b"ACGTNacgtn@+FI:\n") for _ in range(n)]


def _hand(build, **kw):
    b = ic.Bits()
    build(b)
    payload = b.bytes()
    return frame(payload, ic.inflate_raw(payload), **kw), ic.inflate_raw(payload)


def _marker_of_marker(b):
    # 40 000 literals; then, in a block of its own (a run of its own where the chunks are smaller than the first block),
    # a match at distance 32768, whose source lies in the run before, and a copy of that copy
    ic.dynamic_block(b, _noise(40000, 1), final=False)
    ic.dynamic_block(b, [(100, 32768), (50, 60), (258, 150)] + _noise(300, 2), final=False)
    ic.dynamic_block(b, _noise(20, 3), final=True)


def _dist1_fill(b):
    ic.dynamic_block(b, _noise(10000, 4), final=False)
    ic.dynamic_block(b, [(258, 1), (258, 1), (77, 1)] + _noise(40, 5) + [(200, 1)], final=False)
    ic.dynamic_block(b, _noise(20, 6), final=True)


def _too_far(b):
    # the second block reaches one byte before its member's first
    ic.dynamic_block(b, _noise(10000, 7), final=False)
    ic.dynamic_block(b, _noise(10, 8) + [(20, 10012)] + _noise(30, 9), final=False)
    ic.dynamic_block(b, _noise(20, 10), final=True)


@functools.lru_cache(maxsize=None)
def well_formed():
    t, s = text(), small()
    f = {}
    for lvl in (1, 6, 9):
        f["level%d" % lvl] = Fixture(member(t, lvl), t, True)
    f["level0_stored"] = Fixture(member(t, 0), t, True)
    f["fixed"] = Fixture(member(t, 6, zlib.Z_FIXED), t, True)
    f["huffman_only"] = Fixture(member(t, 6, zlib.Z_HUFFMAN_ONLY), t, True)
    f["rle"] = Fixture(member(t, 6, zlib.Z_RLE), t, True)
    f["mem_level1"] = Fixture(member(t, 6, mem_level=1), t, True)
    f["flushes"] = Fixture(frame(_flushed(t[:60000]), t[:60000]), t[:60000], False)
    third = (len(t) // 3) // 4 * 4
    cut = [t.rfind(b"\n@M", 0, third) + 1, t.rfind(b"\n@M", 0, 2 * third) + 1]
    parts = [t[: cut[0]], t[cut[0]: cut[1]], t[cut[1]:]]
    f["three_members"] = Fixture(member(parts[0], 6, fextra=b"XY\x03\x00abc", fname=b"reads_1.fastq") +
                                 member(parts[1], 9, fcomment=b"a comment", fhcrc=True) +
                                 member(parts[2], 1, fextra=b"", fname=b"x", fcomment=b"", fhcrc=True), t, True)
    f["member_end_mid_chunk"] = Fixture(member(s) + member(t[len(s): 100000 + len(s)]), s + t[len(s): 100000 + len(s)], False)
    f["empty_member"] = Fixture(member(s) + member(b"") + member(text(42)[len(s):]), text(42), True)
    f["zero_padding"] = Fixture(member(s) + bytes(64), s, True)
    # what follows the last member and is no member is ignored, as GzInflater ignores it (zlib's gzread does)
    f["bad_magic_second_member"] = Fixture(member(s) + b"\x1f\x8c" + member(s)[2:], s, True)
    f["small"] = Fixture(member(s), s, True)
    for name, build in (("marker_of_marker", _marker_of_marker), ("dist1_fill", _dist1_fill)):
        stream, data = _hand(build)
        f[name] = Fixture(stream, data, False)
    return f


@functools.lru_cache(maxsize=None)
def declined():
    t = text()
    inner = raw(t, 6)                      # real block headers, planted in stored data
    ones = b"A" * 1000000                  # one base repeated: over the ratio cap
    same = (b"@r\n" + b"A" * 91 + b"\n+\n" + b"F" * 91 + b"\n") * 3000   # ... as FASTQ
    # (cut into slices the stored block that a slice cuts off comes first: TRUNCATED, in a run that is not the last)
    return {"stored_of_deflate": (Fixture(member(inner, 0), inner, False), (NO_MEET,)),
            "over_the_ratio_cap": (Fixture(member(ones, 6), ones, False), (REGION,)),
            "fastq_over_the_ratio_cap": (Fixture(member(same, 6), same, True), (REGION,))}


FLIP_BITS = (1, 8 * 2 + 3, 8 * 3 + 6, 8 * 10 + 1, 8 * 10 + 2, 8 * 14 + 5, 8 * 2000 + 3, 8 * 9000 + 7, -8 * 6 + 2, -8 * 2 + 4)


@functools.lru_cache(maxsize=None)
def corrupt():
    """name -> (stream, the statuses the model may end with).  Bit flips at ten fixed places of one member: magic, method,
    reserved flag, block header (twice), code lengths, symbols (twice), CRC, ISIZE (negative: from the end)."""
    t = text()[:60000]
    good = member(t)
    f = {}
    for k, bit in enumerate(FLIP_BITS):
        at = bit if bit >= 0 else 8 * len(good) + bit
        bad = bytearray(good)
        bad[at >> 3] ^= 1 << (at & 7)
        f["flip_%d" % k] = (bytes(bad), None)
    f["wrong_crc"] = (frame(raw(t), t, crc=zlib.crc32(t) ^ 0x10000), (CRC,))
    f["wrong_isize"] = (frame(raw(t), t, isize=len(t) + 1), (ISIZE,))
    f["cut_mid_block"] = (good[: len(good) // 2], (TRUNCATED,))
    b = ic.Bits()
    _too_far(b)
    f["one_byte_too_far_back"] = (frame(b.bytes(), b""), (REACH, DISTANCE))
    return f


# ------------------------------------------------------------------ the model
def build_model(tmp, sanitize=False):
    exe = tmp / ("gzip_model" + ("_asan" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "thermite_amd", "csrc")] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "gzip_model_main.cpp"), "-o", str(exe)])
    return exe


Call = collections.namedtuple("Call", "status bad n last_block n_out n_consumed n_chunks n_starts n_refused n_ends flags paths")
Modelled = collections.namedtuple("Modelled", "calls data states")


def run_model(exe, tmp, chunk, slice_bytes, inputs, last=1, env=None):
    """[(name, stream)] through one run of the program, in the order given -> name -> Modelled: the calls, the inflated
    bytes of all of them, the state (capi.GzipState) after every call that ended with status 0"""
    tag = "%d_%d_%d" % (chunk, slice_bytes, last)
    args = []
    for name, stream in inputs:
        (tmp / (name + ".gz")).write_bytes(stream)
        args += [str(tmp / (name + ".gz")), str(tmp / ("%s.%s.out" % (name, tag)))]
    r = subprocess.run([str(exe), str(chunk), str(slice_bytes), str(last)] + args, capture_output=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr.decode(errors="replace")[-3000:])
    out = {}
    size = capi.C.sizeof(capi.GzipState)
    for name, _ in inputs:
        base = tmp / ("%s.%s.out" % (name, tag))
        calls = [Call(*[int(x) for x in line.split()[1:]]) for line in open(str(base) + ".log").read().splitlines()]
        blob = open(str(base) + ".states", "rb").read()
        states = [capi.GzipState.from_buffer_copy(blob[i: i + size]) for i in range(0, len(blob), size)]
        out[name] = Modelled(calls, base.read_bytes(), states)
        for suffix in ("", ".log", ".states"):
            os.unlink(str(base) + suffix)
    return out


def host_chain(stream, slice_bytes, last=True):
    """the stream through the host path in the calls the model makes -> ([(n, last_block, n_out, n_consumed, state key)],
    the bytes) or, from the call that fails on, the ThermiteError in place of the tuple"""
    st = capi.GzipState()
    at, slice_ = 0, slice_bytes or len(stream)
    calls, data = [], b""
    while True:
        n = min(slice_, len(stream) - at)
        end = at + n == len(stream)
        try:
            got, used = capi.debug_gzip_host_slice(st, stream[at: at + n], last_block=end and last)
        except capi.ThermiteError as e:
            calls.append(e)
            return calls, data
        calls.append((n, int(end and last), len(got), used, st.key()))
        data += got
        at += used
        if end:
            return calls, data
        slice_ = slice_ * 2 if used == 0 else (slice_bytes or len(stream))
