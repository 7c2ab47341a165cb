"""Shared by tests/test_bai_host.py and tests/test_gpu_bai.py: synthetic BAM records with CIGARs, the expectation for the
.bai index (a serial walk of the sorted stream by the rules include/thermite_io.h states above thm_bam_sorter_index), a
parser of .bai files, and a region query written from the SAM specification (sections 4.1, 5.1.1, 5.2, 5.3) that walks a
BGZF file at the chunks an index names.  Nothing here comes from the code under test."""
import struct
import zlib

import numpy as np

CUT = 0xff00
PSEUDO_BIN = 37450
MAX_END = 1 << 29
BOUNDARIES = [1 << 14, 1 << 17, 1 << 20, 1 << 23, 1 << 26]
_HEADER16 = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
OPS = "MIDNSHP=X"


# ------------------------------------------------------------------ records
def make_record(ref_id, pos, flag=0, name=b"r", l_seq=0, cigar=()):
    """a well-formed record: block_size, the fixed fields (bin 4680, whatever the position), the name, the CIGAR words of
    `cigar` = [(op letter or number, length), ...], l_seq bases and qualities"""
    name = bytes(name) + b"\0"
    words = b"".join(struct.pack("<I", n << 4 | (OPS.index(op) if isinstance(op, str) else op)) for op, n in cigar)
    seq = bytes((17 * (i + l_seq)) & 0xff for i in range((l_seq + 1) // 2))
    qual = bytes((i * 7 + pos) & 0x3f for i in range(l_seq))
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name), 0, 4680, len(cigar), flag, l_seq, -1, -1, 0) + name + words + seq + qual
    return struct.pack("<I", len(body)) + body


def sized_record(ref_id, pos, n_bytes, cigar=(("M", 10),), flag=0, tag=b"z"):
    """... of exactly n_bytes bytes (n_bytes >= 300): the name and l_seq make up the length"""
    fixed = 36 + 4 * len(cigar)
    for l_name in range(2, 200):
        rest = n_bytes - fixed - l_name - 1
        l_seq = rest * 2 // 3
        for l in (l_seq - 1, l_seq, l_seq + 1):
            if l >= 0 and (l + 1) // 2 + l == rest:
                rec = make_record(ref_id, pos, flag, tag * l_name, l, cigar)
                assert len(rec) == n_bytes
                return rec
    raise AssertionError(n_bytes)


def split_records(data):
    data = bytes(data)
    out, at = [], 0
    while at < len(data):
        n = 4 + struct.unpack_from("<I", data, at)[0]
        out.append(data[at: at + n])
        at += n
    assert at == len(data)
    return out


def fields(rec):
    """(refID, beg, end, mapped) of one record by the contract; the record's bin field is not read"""
    ref_id, pos, l_name, _, _, n_cig, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    beg = max(pos, 0)
    span = 0
    for w in struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name):
        if OPS[w & 15] in "MDN=X":
            span += w >> 4
    return ref_id, beg, beg + (span or 1), not flag & 4


def reg2bin(beg, end):
    """SAM specification, section 5.3"""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def reg2bins(beg, end):
    """SAM specification, section 5.3: the bins that may hold records overlapping [beg, end)"""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


# ------------------------------------------------------------------ the expectation
def expected_index(stream, n_sq, member_sizes, first_member_offset):
    """the index of the sorted record stream `stream`, as parse_bai gives one back"""
    total = len(stream)
    assert len(member_sizes) == -(-total // CUT)
    coff = [first_member_offset]
    for s in member_sizes:
        coff.append(coff[-1] + int(s))

    def v(s):
        return coff[s // CUT] << 16 | s % CUT

    refs = [dict(bins={}, span=None, n_mapped=0, n_unmapped=0, lin={}, n_intv=0) for _ in range(n_sq)]
    n_no_coor, at, run = 0, 0, None
    for rec in split_records(stream):
        vbeg, vend = v(at), v(at + len(rec))
        at += len(rec)
        ref_id, beg, end, mapped = fields(rec)
        if ref_id < 0:
            n_no_coor += 1
            run = None
            continue
        assert end <= MAX_END
        b = reg2bin(beg, end)
        r = refs[ref_id]
        chunks = r["bins"].setdefault(b, [])
        if run == (ref_id, b):
            chunks[-1][1] = vend               # the run goes on
        elif chunks and chunks[-1][1] >> 16 >= vbeg >> 16:
            chunks[-1][1] = vend               # a new run, merged into the bin's last chunk
        else:
            chunks.append([vbeg, vend])
        run = (ref_id, b)
        r["span"] = [r["span"][0] if r["span"] else vbeg, vend]
        r["n_mapped" if mapped else "n_unmapped"] += 1
        if mapped:
            for w in range(beg >> 14, ((end - 1) >> 14) + 1):
                r["lin"][w] = min(r["lin"].get(w, vbeg), vbeg)
            r["n_intv"] = max(r["n_intv"], ((end - 1) >> 14) + 1)
    out = []
    for r in refs:
        ioffset, above = [0] * r["n_intv"], None
        for w in range(r["n_intv"] - 1, -1, -1):
            above = r["lin"].get(w, above)
            ioffset[w] = above
        assert None not in ioffset
        out.append(dict(bins=[(b, [tuple(c) for c in r["bins"][b]]) for b in sorted(r["bins"])],
                        pseudo=(tuple(r["span"]), (r["n_mapped"], r["n_unmapped"])) if r["span"] else None, ioffset=ioffset))
    return dict(refs=out, n_no_coor=n_no_coor)


def index_bytes(index):
    out = [b"BAI\1", struct.pack("<I", len(index["refs"]))]
    for r in index["refs"]:
        out.append(struct.pack("<I", len(r["bins"]) + (r["pseudo"] is not None)))
        for b, chunks in r["bins"]:
            out.append(struct.pack("<II", b, len(chunks)) + b"".join(struct.pack("<QQ", *c) for c in chunks))
        if r["pseudo"] is not None:
            out.append(struct.pack("<IIQQQQ", PSEUDO_BIN, 2, *r["pseudo"][0], *r["pseudo"][1]))
        out.append(struct.pack("<I", len(r["ioffset"])) + struct.pack("<%dQ" % len(r["ioffset"]), *r["ioffset"]))
    out.append(struct.pack("<Q", index["n_no_coor"]))
    return b"".join(out)


def expected_bai(stream, n_sq, member_sizes, first_member_offset):
    return index_bytes(expected_index(stream, n_sq, member_sizes, first_member_offset))


def parse_bai(data):
    data = bytes(data)
    assert data[:4] == b"BAI\1"
    n_ref, = struct.unpack_from("<I", data, 4)
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<I", data, at)
        at += 4
        bins, pseudo = [], None
        for k in range(n_bin):
            b, n_chunk = struct.unpack_from("<II", data, at)
            at += 8
            chunks = [struct.unpack_from("<QQ", data, at + 16 * c) for c in range(n_chunk)]
            at += 16 * n_chunk
            if b == PSEUDO_BIN:
                assert n_chunk == 2 and k == n_bin - 1, "the pseudo-bin comes last and has two chunks"
                pseudo = (chunks[0], chunks[1])
            else:
                assert b < PSEUDO_BIN - 1
                bins.append((b, chunks))
        n_intv, = struct.unpack_from("<I", data, at)
        at += 4
        ioffset = list(struct.unpack_from("<%dQ" % n_intv, data, at))
        at += 8 * n_intv
        refs.append(dict(bins=bins, pseudo=pseudo, ioffset=ioffset))
    n_no_coor, = struct.unpack_from("<Q", data, at)
    assert at + 8 == len(data), "bytes behind n_no_coor"
    return dict(refs=refs, n_no_coor=n_no_coor)


def counts(index):
    """what thm_bai_view counts: n_bins with the pseudo-bins, n_chunks of the other bins"""
    refs = index["refs"]
    return dict(n_refs=len(refs), n_bins=sum(len(r["bins"]) + (r["pseudo"] is not None) for r in refs),
                n_chunks=sum(len(c) for r in refs for _, c in r["bins"]), n_intervals=sum(len(r["ioffset"]) for r in refs),
                n_no_coor=index["n_no_coor"])


# ------------------------------------------------------------------ a BGZF file and the query
def bgzf_member(raw):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    payload = c.compress(raw) + c.flush()
    return _HEADER16 + struct.pack("<H", len(payload) + 25) + payload + struct.pack("<II", zlib.crc32(raw), len(raw))


def bgzf_members(stream):
    """the stream cut every 0xff00 bytes, every piece a BGZF member (zlib's) -> the members"""
    return [bgzf_member(stream[at: at + CUT]) for at in range(0, len(stream), CUT)]


class BgzfFile:
    """random access by virtual offset (SAM specification, section 4.1.1)"""

    def __init__(self, data):
        self.data, self.cache = bytes(data), {}

    def block(self, coff):
        if coff not in self.cache:
            assert self.data[coff: coff + 16] == _HEADER16, "no BGZF member at %d" % coff
            size = struct.unpack_from("<H", self.data, coff + 16)[0] + 1
            self.cache[coff] = (zlib.decompress(self.data[coff + 18: coff + size - 8], -15), size)
        return self.cache[coff]

    def read(self, v, n):
        """n bytes from virtual offset v -> (bytes, the virtual offset behind them: at the end of a block, the next block's)"""
        coff, uoff, out = v >> 16, v & 0xffff, []
        while True:
            blk, size = self.block(coff)
            if uoff >= len(blk) and coff + size < len(self.data):
                coff, uoff = coff + size, 0
                continue
            if n == 0:
                return b"".join(out), coff << 16 | uoff
            assert uoff < len(blk), "read beyond the end of the file"
            take = blk[uoff: uoff + n]
            out.append(take)
            n -= len(take)
            uoff += len(take)


def query(index, bam, ref, beg, end):
    """the records of BGZF file `bam` on reference `ref` that overlap [beg, end), found through `index` (parse_bai's): the
    bins that overlap the region, their chunks whose end is above the linear index's offset for beg, the records at those
    chunks, filtered by overlap"""
    r = index["refs"][ref]
    wanted = set(reg2bins(beg, end))
    w = beg >> 14
    min_off = r["ioffset"][w] if w < len(r["ioffset"]) else (r["ioffset"][-1] if r["ioffset"] else 0)
    f = bam if isinstance(bam, BgzfFile) else BgzfFile(bam)
    # a merged chunk of one bin may span records of another bin: the chunks are put in file order and overlapping ones
    # joined before the file is read, so that no record comes twice
    todo = []
    for cbeg, cend in sorted(c for b, chunks in r["bins"] if b in wanted for c in chunks if c[1] > min_off):
        if todo and cbeg <= todo[-1][1]:
            todo[-1][1] = max(todo[-1][1], cend)
        else:
            todo.append([cbeg, cend])
    out = []
    for cbeg, cend in todo:
        v = cbeg
        while v < cend:
            head, v = f.read(v, 4)
            body, v = f.read(v, struct.unpack("<I", head)[0])
            rec = head + body
            ref_id, rbeg, rend, _ = fields(rec)
            if ref_id == ref and rbeg < end and rend > beg:
                out.append(rec)
    return out


def brute_force(stream, ref, beg, end, mapped_only=True):
    out = []
    for rec in split_records(stream):
        ref_id, rbeg, rend, mapped = fields(rec)
        if ref_id == ref and rbeg < end and rend > beg and (mapped or not mapped_only):
            out.append(rec)
    return out


def mapped(records):
    return [rec for rec in records if fields(rec)[3]]


def regions_of(stream, n_sq):
    """(ref, beg, end) to query: the whole reference, a single base at and either side of both ends of some records, each
    side of every bin boundary, a region between records that none overlaps, one beyond the last"""
    by_ref = {}
    for rec in split_records(stream):
        ref_id, beg, end, _ = fields(rec)
        if ref_id >= 0:
            by_ref.setdefault(ref_id, []).append((beg, end))
    out = []
    for ref in range(n_sq):
        iv = sorted(by_ref.get(ref, []))
        out.append((ref, 0, MAX_END))
        if not iv:
            out.append((ref, 100, 200))
            continue
        for b in BOUNDARIES:
            out += [(ref, b - 1, b), (ref, b, b + 1), (ref, b - 1, b + 1)]
        for beg, end in (iv[0], iv[len(iv) // 2], iv[-1]):
            out += [(ref, beg, beg + 1), (ref, end - 1, end), (ref, end, end + 1)] + ([(ref, beg - 1, beg)] if beg else [])
        reach, gap = 0, None
        for beg, end in iv:
            if gap is None and reach and beg - reach >= 3:
                gap = (ref, reach + 1, beg - 1)
            reach = max(reach, end)
        if gap:
            out.append(gap)
        out.append((ref, reach + 10, reach + 20))
    return out


def check_queries(index, bam, stream, n_sq, regions=None):
    """query() through `index` finds, in every region, exactly the mapped records a walk of the whole stream finds"""
    f = BgzfFile(bam)
    for ref, beg, end in regions or regions_of(stream, n_sq):
        assert mapped(query(index, f, ref, beg, end)) == brute_force(stream, ref, beg, end), (ref, beg, end)


# ------------------------------------------------------------------ the cases
W = 1 << 14


def synthetic_cases(n_sq=4):
    """name -> records in any order (the sort comes first): the smallest shapes at which a pass of the index can go wrong"""
    rng = np.random.default_rng(0xBA1)
    cases = {"empty": b""}
    # records on reference 2 only, and some without a reference
    recs = [make_record(2, int(rng.integers(0, 200000)), int(rng.integers(0, 2)) * 16, b"o%d" % i, int(rng.integers(0, 40)),
                        [("M", int(rng.integers(30, 150)))]) for i in range(300)]
    recs += [make_record(-1, -1, 4, b"u%d" % i, 20) for i in range(20)]
    cases["one_reference"] = b"".join(recs[i] for i in rng.permutation(len(recs)))
    # every level of the binning: ending on a boundary (stays in the lower-level bin), crossing it by one base, starting on it
    recs = []
    for k, b in enumerate(BOUNDARIES):
        for ref in (0, 1):
            recs += [make_record(ref, b - 100, 0, b"on%d" % k, 10, [("M", 100)]), make_record(ref, b - 100, 0, b"x%d" % k, 10, [("M", 60), ("D", 41)]),
                     make_record(ref, b, 16, b"at%d" % k, 10, [("=", 50), ("X", 50)])]
    cases["bin_levels"] = b"".join(recs[i] for i in rng.permutation(len(recs)))
    # no reference span: end = beg + 1
    recs = [make_record(0, 5000, 0, b"nocigar", 10), make_record(0, W - 1, 0, b"clips", 30, [("S", 10), ("I", 5), ("H", 3), ("P", 2), ("S", 15)]),
            make_record(1, -1, 0, b"posm1", 8), make_record(1, -1, 16, b"posm1r", 8), make_record(0, 3 * W, 0, b"plain", 12, [("M", 12)]),
            make_record(3, W, 0, b"empty_ops", 4, [("M", 0), ("S", 4)])]
    cases["no_span"] = b"".join(recs)
    # the linear index: an N op over 5 windows, two populated windows 40 empty ones apart, placed unmapped records alone in
    # a window (one among the empty windows, one above every mapped record)
    recs = [make_record(0, 20000, 0, b"spliced", 20, [("M", 10), ("N", 70000), ("M", 10)]), make_record(0, 30000, 0, b"in", 20, [("M", 20)]),
            make_record(0, 100 * W + 5, 0, b"low", 20, [("M", 20)]), make_record(0, 141 * W + 5, 16, b"high", 20, [("M", 20)]),
            make_record(0, 120 * W + 7, 4, b"un_mid", 20), make_record(0, 200 * W + 7, 4 | 16, b"un_top", 20, [("M", 20)]),
            make_record(1, 2 * W + 1, 4, b"only_unmapped", 20)]
    cases["linear"] = b"".join(recs)
    # the merge rule: records of a 16 kb bin interleaved with records of its parent bin that cross into the next window.
    # Reference 0: so densely that the parent's chunks share a member; reference 1: 90 kB of leaf records between them.
    recs, base = [], 5 * W - 30
    for k in range(20):
        recs += [make_record(0, base + k, 0, b"par%d" % k, 30, [("M", 50)]), make_record(0, base + k, 0, b"leaf%d" % k, 30, [("M", 5)])]
    for k in range(4):
        recs += [make_record(1, base + k, 0, b"par%d" % k, 30, [("M", 50)]), make_record(1, base + k, 0, b"leafa%d" % k, 30000, [("M", 5)]),
                 make_record(1, base + k, 0, b"leafb%d" % k, 30000, [("M", 5)])]
    cases["merge"] = b"".join(recs)
    # member cuts: the first sorted record is exactly one member long, so the second begins on a cut; a record longer than a
    # member in the middle of a bin's run; the last record pads the stream to a multiple of 0xff00
    recs = [sized_record(0, 10, CUT)]
    recs += [make_record(0, 1000 + i, 0, b"a%d" % i, 50, [("M", 50)]) for i in range(40)]
    recs += [make_record(0, 1040, 0, b"long", 46000, [("M", 80)])]
    recs += [make_record(0, 1041 + i, 16, b"b%d" % i, 50, [("M", 50)]) for i in range(40)]
    recs += [make_record(2, 70000 + 300 * i, 0, b"c%d" % i, 100, [("M", 100)]) for i in range(300)]
    n = sum(len(r) for r in recs)
    recs.append(sized_record(3, 77, CUT - n % CUT + (CUT if CUT - n % CUT < 300 else 0)))
    cases["member_cuts"] = b"".join(recs)
    assert len(cases["member_cuts"]) % CUT == 0
    # 70 000 short records over a few hundred bins: every scan, compaction and sort spans several workgroups and tiles
    ref = np.sort(rng.integers(0, n_sq, 70000))
    pos = rng.integers(0, 120 * W, 70000)
    ln = rng.integers(1, 3000, 70000)
    fl = rng.integers(0, 40, 70000)
    cases["many"] = b"".join(make_record(int(ref[i]) if fl[i] != 7 else -1, int(pos[i]), 4 if fl[i] == 3 else (16 if fl[i] & 1 else 0), b"m",
                                         0, [("M", int(ln[i]))]) for i in range(70000))
    return cases
