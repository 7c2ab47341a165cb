"""Shared by tests/test_inflate_device_host.py and tests/test_gpu_inflate_device.py: the gzip members the device BGZF
inflater (thermite_amd/csrc/inflate_device.h, kernels_inflate.hip, thm_batch_upload_fastq_bgzf) is checked on.  The
reference for the bytes is gzip.decompress / zlib of the standard library; for batches and errors it is the host path,
GzInflater plus fastq_parse_block (fastq_device_common.host_outcome on the members written out as a .fastq.gz file).

well_formed():  name -> Fixture: members the device must inflate, every one of them (no decline is allowed)
not_for_device(): valid gzip the walk turns away; the host inflater's bytes are the result
corrupt():      members that end with a status word (or fail the walk) and then with the host inflater's ERR_IO

Members are built with zlib.compressobj(level, DEFLATED, -15, 9, strategy) plus the 18-byte BGZF header and the trailer;
what zlib never emits (a distance of 32768, a match of 258 at distance 32506, unassigned codes, ...) is assembled by the
bit writer below and checked against zlib.decompressobj(-15) where it is well formed."""
import collections
import heapq
import struct
import zlib

import numpy as np

Fixture = collections.namedtuple("Fixture", "members data fastq")   # fastq: the inflated bytes are whole FASTQ records

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
# status words and path bits of inflate_device.h
OK, TRUNCATED, BLOCK_TYPE, STORED_LEN, CODE_LENGTHS, BAD_CODE, DISTANCE, OUTPUT, CRC, TABLE_ROOM, TRAILING, MEMBER = range(12)
P_STORED, P_FIXED, P_DYNAMIC, P_SUBTABLE, P_OVERLAP, P_FAR, P_MULTIBLOCK = 1, 2, 4, 8, 16, 32, 64
PATH_NAMES = {P_STORED: "stored", P_FIXED: "fixed", P_DYNAMIC: "dynamic", P_SUBTABLE: "sub-table", P_OVERLAP: "overlapping copy",
              P_FAR: "distance over 16384", P_MULTIBLOCK: "multi-block"}


def host_outcome_gz(tmp_path, name, members):
    """(('batch', dict) | ('error', code, message), path): what the host path -- GzInflater, then fastq_parse_block over
    the whole text as one block -- makes of the members written out as tmp_path/name.fastq.gz"""
    import fastq_device_common as fc
    from thermite_amd import capi
    p = tmp_path / (name + ".fastq.gz")
    p.write_bytes(members)
    try:
        return ("batch", fc.host_parse(p)), str(p)
    except capi.ThermiteError as e:
        return ("error", e.code, fc.message(e)), str(p)


# ------------------------------------------------------------------ framing
def frame(payload, data=b"", crc=None, isize=None, bsize=None, flg=4, extra=None, name=b""):
    """payload (a raw DEFLATE stream) as a gzip member with the BGZF header; the keyword arguments bend it"""
    total = 12 + (6 if extra is None else len(extra)) + len(name) + len(payload) + 8
    if extra is None:
        extra = b"BC\x02\x00" + struct.pack("<H", (total - 1 if bsize is None else bsize) & 0xFFFF)
    head = b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff" + (struct.pack("<H", len(extra)) + extra if flg & 4 else b"")
    return head + name + payload + struct.pack("<II", zlib.crc32(data) if crc is None else crc, len(data) if isize is None else isize)


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, flush=zlib.Z_FULL_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(flush) + c.compress(data[flush_at:]) + c.flush()


def member(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **kw):
    m = frame(raw_deflate(data, level, strategy, kw.pop("flush_at", None), kw.pop("flush", zlib.Z_FULL_FLUSH)), data, **kw)
    return m


def members_of(data, cut, level=6):
    """data cut every `cut` bytes, a BGZF member each"""
    return b"".join(member(data[i: i + cut], level) for i in range(0, len(data), cut))


# ------------------------------------------------------------------ a bit writer and the two code kinds
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):          # n bits, least significant first (header fields, extra bits)
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):         # a Huffman code, most significant bit first
        self.put(int(format(c, "0%db" % n)[::-1], 2), n)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
              8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def len_symbol(length):
    k = 28 if length == 258 else max(i for i in range(28) if _LEN_BASE[i] <= length)
    return 257 + k, _LEN_EXTRA[k], length - _LEN_BASE[k]


def dist_symbol(dist):
    k = max(i for i in range(30) if _DIST_BASE[i] <= dist)
    return k, _DIST_EXTRA[k], dist - _DIST_BASE[k]


def fixed_code(sym):
    if sym < 144:
        return 0x30 + sym, 8
    if sym < 256:
        return 0x190 + sym - 144, 9
    if sym < 280:
        return sym - 256, 7
    return 0xC0 + sym - 280, 8


def canonical(lens):
    """code lengths -> {symbol: (code, length)}"""
    count = collections.Counter(l for l in lens if l)
    code, nxt = 0, {}
    for l in range(1, 16):
        code = (code + count.get(l - 1, 0)) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def huffman_lens(freq, n):
    """a complete code over the symbols with freq > 0 (two at least); few symbols, so no length limit is met"""
    heap = [(f, s, (s,)) for s, f in sorted(freq.items()) if f > 0]
    assert len(heap) >= 2
    heapq.heapify(heap)
    lens = [0] * n
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            lens[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    assert max(lens) <= 15
    return lens


def put_tokens(b, tokens, lit, dist):
    """tokens: a literal byte, or (length, distance), or ('sym', literal/length symbol), or ('dsym', length, distance code)"""
    for t in tokens:
        if isinstance(t, int):
            b.code(*lit[t])
        elif t[0] == "sym":
            b.code(*lit[t[1]])
        else:
            ls, ln, lx = len_symbol(t[1] if t[0] == "dsym" else t[0])
            b.code(*lit[ls])
            b.put(lx, ln)
            if t[0] == "dsym":
                b.code(*dist[t[2]])
            else:
                ds, dn, dx = dist_symbol(t[1])
                b.code(*dist[ds])
                b.put(dx, dn)


_FIXED_LIT = {s: fixed_code(s) for s in range(288)}
_FIXED_DIST = {s: (s, 5) for s in range(32)}


def fixed_block(b, tokens, final=True, eob=True):
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    put_tokens(b, tokens, _FIXED_LIT, _FIXED_DIST)
    if eob:
        b.code(*_FIXED_LIT[256])


def stored_block(b, data, final=False, nlen=None):
    b.put(1 if final else 0, 1)
    b.put(0, 2)
    b.align()
    b.put(len(data), 16)
    b.put((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
    b.out += data


def dynamic_header(b, final, lit_lens, dist_lens, cl_lens=None, cl_syms=None):
    """the lengths written one code-length symbol each (every code-length code 4 bits: symbols 0..15), unless cl_lens /
    cl_syms (a list of (symbol, extra value)) say otherwise"""
    hlit = max(257, max(i for i, l in enumerate(lit_lens) if l) + 1)
    hdist = max(1, max([i for i, l in enumerate(dist_lens) if l] + [0]) + 1)
    if cl_lens is None:
        cl_lens = [4] * 16 + [0, 0, 0]
    if cl_syms is None:
        cl_syms = [(l, 0) for l in list(lit_lens[:hlit]) + list(dist_lens[:hdist])]
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(hlit - 257, 5)
    b.put(hdist - 1, 5)
    b.put(19 - 4, 4)
    for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
        b.put(cl_lens[s], 3)
    cl = canonical(cl_lens)
    for s, x in cl_syms:
        b.code(*cl[s])
        if s >= 16:
            b.put(x, {16: 2, 17: 3, 18: 7}[s])


def dynamic_block(b, tokens, final=True, dist_lens=None):
    lf, df = collections.Counter({256: 1}), collections.Counter()
    for t in tokens:
        if isinstance(t, int):
            lf[t] += 1
        else:
            lf[len_symbol(t[0])[0]] += 1
            df[dist_symbol(t[1])[0]] += 1
    if len(lf) < 2:
        lf[0] += 1
    lit_lens = huffman_lens(lf, 286)
    if dist_lens is None:
        if len(df) >= 2:
            dist_lens = huffman_lens(df, 30)
        else:   # one distance code of one bit, or none in use
            dist_lens = [0] * 30
            dist_lens[next(iter(df), 0)] = 1
    dynamic_header(b, final, lit_lens, dist_lens)
    put_tokens(b, tokens, canonical(lit_lens), canonical(dist_lens))
    b.code(*canonical(lit_lens)[256])


def inflate_raw(payload):
    d = zlib.decompressobj(-15)
    out = d.decompress(payload)
    assert d.eof and not d.unused_data
    return out


def hand(build, **kw):
    """a member around the stream `build` writes into a Bits; the data is what zlib makes of it"""
    b = Bits()
    build(b)
    payload = b.bytes()
    return frame(payload, inflate_raw(payload), **kw)


# ------------------------------------------------------------------ texts
def fastq_text(n_bytes, seed=3, read_len=(30, 151)):
    """whole 4-line records, n_bytes exactly (the last name is padded to the byte)"""
    rng = np.random.default_rng(seed)
    out, size, i = [], 0, 0
    alpha = np.frombuffer(b"ACGTN", np.uint8)
    while True:
        L = int(rng.integers(*read_len))
        idx = rng.integers(0, 4, L)
        idx[rng.integers(0, 50, L) == 0] = 4
        seq = bytes(alpha[idx])
        qual = bytes(np.repeat(rng.integers(35, 74, L // 8 + 1).astype(np.uint8), 8)[:L])
        rec = b"@SIM:%d:FC:1:%d:%d 1:N:0\n" % (seed, 1000 + i, 7 * i) + seq + b"\n+\n" + qual + b"\n"
        if size + len(rec) + 12 > n_bytes:
            break
        out.append(rec)
        size += len(rec)
        i += 1
    pad = n_bytes - size
    assert pad >= 12
    out.append(b"@" + b"p" * (pad - 10) + b"\nAC\n+\nII\n")
    text = b"".join(out)
    assert len(text) == n_bytes
    return text


def fibonacci_bytes():
    """byte values with Fibonacci frequencies, spread: under Z_HUFFMAN_ONLY the rare ones get codes of 15 bits"""
    fib = [1, 1]
    while len(fib) < 22:   # 46367 bytes in all
        fib.append(fib[-1] + fib[-2])
    data = np.concatenate([np.full(f, 65 + k, np.uint8) for k, f in enumerate(fib)])
    np.random.default_rng(8).shuffle(data)
    return data.tobytes()


def far_tokens(first=32768, total=65536):
    """behind `first` literal bytes: matches of 258 and 3 at distances 32768, 32506 and 1, then matches of 258 at
    distance 32768 up to `total` bytes"""
    toks = [(258, 32768), (3, 32768), (258, 32506), (3, 32506), (3, 1), (258, 1)]
    left = total - first - sum(t[0] for t in toks)
    while left >= 258 + 3:
        toks.append((258, 32768))
        left -= 258
    if left > 258:
        toks.append((130, 32768))
        left -= 130
    assert 3 <= left <= 258
    toks.append((left, 32768))
    return toks


# ------------------------------------------------------------------ the fixtures
_cache = {}


def well_formed():
    if "well" in _cache:
        return _cache["well"]
    rng = np.random.default_rng(21)
    out = {}

    def add(name, members, fastq=False):
        data = b"".join(zlib.decompress(m, 31) for m in split_members(members))
        out[name] = Fixture(members, data, fastq)

    t3000, t39k, t20k = fastq_text(3000, 4), fastq_text(39000, 5), fastq_text(20000, 6)
    rand = rng.integers(0, 256, 65436).astype(np.uint8).tobytes()
    # stored
    add("stored_3000", member(t3000, 0), True)
    add("stored_65436_random", member(rand, 0))
    add("stored_two_blocks", member(rand[:40000], 0, flush_at=20000))
    add("stored_block_of_length_0", member(t3000, 6, flush_at=1500, flush=zlib.Z_SYNC_FLUSH), True)
    # fixed
    add("fixed_3000_fastq", member(t3000, 6, zlib.Z_FIXED), True)
    add("empty_member", EOF_BLOCK)
    add("one_byte", member(b"A", 6, zlib.Z_FIXED))
    # dynamic
    for level in (1, 6, 9):
        add("dynamic_fastq_level_%d" % level, member(t39k, level), True)
    add("fibonacci_code_length_15", member(fibonacci_bytes(), 9, zlib.Z_HUFFMAN_ONLY))
    add("full_flush_mid_member", member(t39k, 6, flush_at=17001), True)
    abc = [97, 98, 99, 100, 101, 102] + [(6, 6), (4, 5), (3, 6), (5, 5)] * 9 + [10]
    add("single_distance_code", hand(lambda b: dynamic_block(b, abc)))
    # copies
    add("run_of_5000", member(b"F" * 5000))
    for period in (2, 3, 63, 64, 65):
        unit = rng.integers(33, 127, period).astype(np.uint8).tobytes()
        add("period_%d" % period, member((unit * (4000 // period + 2))[:4001]))
    first = rng.integers(0, 256, 32768).astype(np.uint8).tobytes()

    def far(block):
        def build(b):
            stored_block(b, first)
            block(b, far_tokens())
        return build
    add("hand_matches_fixed_65536", hand(far(fixed_block)))
    add("hand_matches_dynamic_65536", hand(far(dynamic_block)))
    # sizes (0 and 1 above)
    add("isize_ff00", member(fastq_text(0xff00, 7)), True)
    add("isize_65536", member(fastq_text(65536, 9)), True)
    # member counts
    add("two_members", members_of(t20k, 10000), True)
    add("members_65", members_of(t20k, -(-len(t20k) // 65)), True)
    t40 = b"@a b\nACGTNACGTA\n+\nIIIIIFFFF#\n@c\nAC\n+\n!~\n"
    assert len(t40) == 40
    add("one_byte_members_40", members_of(t40, 1), True)
    add("cut_every_100", members_of(t20k, 100), True)
    assert len(split_members(out["members_65"].members)) == 65
    _cache["well"] = out
    return out


def split_members(members):
    """BGZF members back to back -> a list of them (by BSIZE; every fixture of well_formed() has the 18-byte header)"""
    out, at = [], 0
    while at < len(members):
        assert members[at: at + 4] == b"\x1f\x8b\x08\x04" and members[at + 12: at + 16] == b"BC\x02\x00"
        size = struct.unpack_from("<H", members, at + 16)[0] + 1
        out.append(members[at: at + size])
        at += size
    assert at == len(members)
    return out


def not_for_device():
    """name -> Fixture: valid gzip that the walk turns away; the inflate is the host's and the result is still right"""
    import gzip
    text = fastq_text(3000, 4)
    big = fastq_text(70000, 12)
    two = member(text[:1512]) + gzip.compress(text[1512:], mtime=0)
    rnd = np.random.default_rng(22).integers(0, 256, 65536).astype(np.uint8).tobytes()
    return {
        "plain_gzip_member": Fixture(gzip.compress(text, mtime=0), text, True),
        "fextra_without_bc": Fixture(member(text, extra=b"XY\x02\x00\x01\x02"), text, True),
        "fname_set": Fixture(member(text, flg=4 | 8, name=b"reads.fastq\0"), text, True),
        "isize_over_65536": Fixture(member(big), big, True),
        "bgzf_member_then_a_plain_one": Fixture(two, text, True),
        "stored_65536_plain_gzip": Fixture(gzip.compress(rnd, 0, mtime=0), rnd, False),
        "bsize_40_short": Fixture(_bsize_short(member(text), 40), text, True),
    }


def _bsize_short(m, by):
    """BSIZE says the member ends `by` bytes early: the chain does not hold, the stream itself is whole"""
    m = bytearray(m)
    struct.pack_into("<H", m, 16, len(m) - 1 - by)
    return bytes(m)


def corrupt():
    """name -> (members, the status words the model may end the first bad member with; None: the walk fails)"""
    text = fastq_text(3000, 4)
    payload = raw_deflate(text)
    out = {}
    out["crc_flipped"] = (frame(payload, text, crc=zlib.crc32(text) ^ 0x10), {CRC})
    out["isize_one_too_small"] = (frame(payload, text, isize=len(text) - 1), {OUTPUT})
    out["isize_one_too_large"] = (frame(payload, text, isize=len(text) + 1), {OUTPUT})
    # the payload ten bytes short, BSIZE in keeping: what the cut leaves of the last symbol may decode as anything
    out["payload_truncated_by_bsize"] = (frame(payload[:-10], text), {TRUNCATED, BAD_CODE, DISTANCE, OUTPUT})

    def h(build, data=b"", **kw):
        b = Bits()
        build(b)
        return frame(b.bytes(), data, **kw)

    def type3(b):
        b.put(1, 1)
        b.put(3, 2)
    out["block_type_3"] = (h(type3), {BLOCK_TYPE})
    lit_ok = huffman_lens({65: 5, 66: 3, 256: 1}, 286)
    over = list(lit_ok)
    over[67] = over[68] = 1     # two more codes of one bit: more codes than the lengths leave room for
    out["oversubscribed_code_lengths"] = (h(lambda b: dynamic_header(b, True, over, [1] + [0] * 29)), {CODE_LENGTHS})
    rep_first = [4] * 15 + [0, 5, 5, 0]   # symbols 0..14 of four bits, 16 and 17 of five: a complete code
    out["repeat_with_nothing_before_it"] = (h(lambda b: dynamic_header(b, True, lit_ok, [1] + [0] * 29, rep_first, [(16, 0), (8, 0)])),
                                            {CODE_LENGTHS})
    out["literal_length_symbol_286"] = (h(lambda b: fixed_block(b, [65, ("sym", 286), 66]), b"AB"), {BAD_CODE})
    out["distance_code_30"] = (h(lambda b: fixed_block(b, [65, 66, 67, ("dsym", 3, 30)]), b"ABCABC"), {BAD_CODE})
    out["distance_beyond_the_bytes_produced"] = (h(lambda b: fixed_block(b, [65, (3, 2)]), b"AAAA"), {DISTANCE})
    out["len_nlen_mismatch"] = (h(lambda b: stored_block(b, b"hello", True, nlen=0x1234), b"hello"), {STORED_LEN})
    out["no_end_of_block"] = (h(lambda b: fixed_block(b, [65] * 9, eob=False), b"A" * 9), {TRUNCATED})
    out["output_past_isize"] = (h(lambda b: fixed_block(b, [65, 66, 67, 68, (200, 4)]), b"ABCD" * 20), {OUTPUT})
    return out
