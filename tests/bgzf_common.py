"""Shared by tests/test_bgzf_host.py and tests/test_gpu_bgzf.py: the decoder every BGZF member of the device encoder
goes through (written here from the SAM specification, section 4.1, and RFC 1951/1952; inflation by Python's zlib),
and the byte strings the encoder's edge cases are made of."""
import struct
import zlib

import numpy as np

BLOCK_IN = 0xff00
HEADER16 = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def check_blocks(data, block_off=None, full=True):
    """Walks the members (by block_off, or by BSIZE when there is none) -> (inflated stream, [payload bytes per member],
    [member is a stored block]).  Asserts for every member: the 18 header bytes, BSIZE + 1 == its length, a raw DEFLATE
    stream that ends exactly at the 8-byte tail, CRC-32 and ISIZE; every member but the last inflates to 0xff00 bytes
    (full=False: members of any size, as in a file of several batches)."""
    data = bytes(data)
    if block_off is None:
        block_off, at = [0], 0
        while at < len(data):
            assert len(data) - at >= 28, "trailing bytes"
            at += struct.unpack_from("<H", data, at + 16)[0] + 1
            block_off.append(at)
    block_off = [int(x) for x in block_off]
    assert block_off[0] == 0 and block_off[-1] == len(data)
    out, payload, stored = [], [], []
    for b in range(len(block_off) - 1):
        m = data[block_off[b]: block_off[b + 1]]
        assert len(m) >= 28 and m[:16] == HEADER16, "member %d: header" % b
        bsize, = struct.unpack_from("<H", m, 16)
        assert bsize + 1 == len(m), "member %d: BSIZE %d, length %d" % (b, bsize, len(m))
        d = zlib.decompressobj(-15)
        x = d.decompress(m[18:-8]) + d.flush()
        assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", "member %d: the payload does not end at the tail" % b
        crc, isize = struct.unpack_from("<II", m, len(m) - 8)
        assert crc == zlib.crc32(x) and isize == len(x), "member %d: CRC-32 or ISIZE" % b
        out.append(x)
        payload.append(len(m) - 26)
        stored.append((m[18] & 7) == 1)   # BFINAL = 1, BTYPE = 00
    assert not full or all(len(x) == BLOCK_IN for x in out[:-1]), "a member before the last is not 0xff00 bytes"
    return b"".join(out), payload, stored


def zlib1_payload(raw):
    """total bytes of zlib level 1 raw DEFLATE streams over the same 0xff00-byte cuts"""
    total = 0
    for at in range(0, len(raw), BLOCK_IN):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        total += len(c.compress(raw[at: at + BLOCK_IN]) + c.flush())
    return total


def edge_cases():
    """name -> bytes: the inputs of the encoder's edge cases (tests/test_gpu_bgzf.py lists what each is for)"""
    rng = np.random.default_rng(0xb62f)
    rnd = lambda n: bytes(rng.integers(0, 256, n).astype(np.uint8))
    cases = {}
    for n in (0, 1, 3, 4, 5, BLOCK_IN - 1, BLOCK_IN, BLOCK_IN + 1, 2 * BLOCK_IN, 3 * BLOCK_IN + 17):
        cases["len_%d" % n] = bytes((rng.integers(0, 4, n) + 65).astype(np.uint8))   # four letters: compressible
    cases["zeros"] = bytes(BLOCK_IN)
    cases["one_byte_x7"] = b"q" * 7
    cases["all_256_once"] = bytes(range(256))
    # every 4-gram over four letters exactly once (a de Bruijn sequence): no match either, but two bits a literal, so
    # the dynamic block is kept and its distance alphabet has no used code
    seq, a = [], [0] * 16

    def db(t, p):
        if t > 4:
            if 4 % p == 0:
                seq.extend(a[1: p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 4):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    cases["de_bruijn_4_4"] = bytes(b"ACGT"[x] for x in seq + seq[:3])
    cases["random"] = rnd(2 * BLOCK_IN + 1000)
    cases["motif_200"] = rnd(200) * 300
    s = rnd(32768)
    cases["twice_32768"] = s + s
    s = rnd(32769)
    cases["twice_32769"] = s + s
    cases["period_1019"] = rnd(1019) * 64
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    p = np.array(fib, float)
    cases["fibonacci"] = bytes((rng.choice(30, 60000, p=p / p.sum()) + 40).astype(np.uint8))
    return cases
