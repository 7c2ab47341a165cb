"""What the cell-by-gene UMI matrix of a run must hold (include/thermite_io.h, above thm_cells_create), written from that
contract alone in plain Python: `parse_tag` reads barcode and UMI off a name, `expected` classifies the reads of a view
into the molecule dict and the totals, `rows` cuts the cells and entries of a fetch out of the molecules, `mtx_of` gives the
driver's three files.  `gen_names` draws read names from small pools of barcodes and UMIs.  Nothing here touches the
library under test."""
import numpy as np

from thermite_amd import capi

TOTAL_NAMES = ["n_reads", "n_failed_reads", "n_unmapped_reads", "n_multi_reads", "n_intergenic_reads", "n_intronic_skipped_reads",
               "n_untagged_reads", "n_counted_reads"]
CELL_DT = np.dtype([("n_reads", "<u8"), ("barcode", "<u4"), ("n_umis", "<u4"), ("n_genes", "<u4"), ("pad_", "<u4")])
ENTRY_DT = np.dtype([("cell", "<u4"), ("gene", "<u4"), ("n_umis", "<u4"), ("n_reads", "<u4")])
EXONIC, INTRONIC, INTERGENIC = 0, 1, 2
INTRONIC_FLAG = 1
_CODE = {65: 0, 67: 1, 71: 2, 84: 3}   # upper-case A C G T only


# ------------------------------------------------------------------ the tag
def pack(seq):
    """bytes of upper-case ACGT -> the packed integer, first base most significant; None where a byte is anything else"""
    v = 0
    for c in seq:
        if c not in _CODE:
            return None
        v = v << 2 | _CODE[c]
    return v


def unpack(v, n):
    return "".join("ACGT"[(v >> (2 * (n - 1 - i))) & 3] for i in range(n))


def parse_tag(name, cb_len, umi_len):
    """the name of a read (bytes) -> (barcode, umi) packed, or None: QNAME is the name up to its first space; its last
    cb_len + umi_len + 2 bytes must be '_' barcode '_' umi"""
    q = bytes(name).split(b" ", 1)[0]
    need = cb_len + umi_len + 2
    if len(q) < need:
        return None
    tag = q[len(q) - need:]
    if tag[0:1] != b"_" or tag[1 + cb_len: 2 + cb_len] != b"_":
        return None
    bc, umi = pack(tag[1: 1 + cb_len]), pack(tag[2 + cb_len:])
    if bc is None or umi is None:
        return None
    return bc, umi


# ------------------------------------------------------------------ the molecules of a view
def split_names(names, name_off):
    names = bytes(np.ascontiguousarray(names, np.uint8)) if not isinstance(names, (bytes, bytearray)) else bytes(names)
    return [names[int(name_off[i]): int(name_off[i + 1])] for i in range(len(name_off) - 1)]


def join_names(names):
    """a list of names -> (pool as uint8, offsets)"""
    return np.frombuffer(b"".join(names), np.uint8), np.cumsum([0] + [len(n) for n in names]).astype("<u8")


def expected(t, offsets, alns, status, names, name_off, flags, cb_len, umi_len):
    """-> ({(barcode, gene, umi): reads}, totals dict): every read falls into exactly one total, tested in the contract's order"""
    tot = dict.fromkeys(TOTAL_NAMES, 0)
    mol = {}
    offsets = [int(x) for x in offsets]
    nm = split_names(names, name_off)
    tx_gene = [int(g) for g in t["txs"]["gene_idx"]]
    for r in range(len(offsets) - 1):
        nh = offsets[r + 1] - offsets[r]
        tot["n_reads"] += 1
        if status is not None and int(status[r]) != 0:
            tot["n_failed_reads"] += 1
            continue
        if nh == 0:
            tot["n_unmapped_reads"] += 1
            continue
        if nh > 1:
            tot["n_multi_reads"] += 1
            continue
        al = alns[offsets[r]]
        ty, idx = int(al["aln_type"]), int(al["tx_or_gene_idx"])
        if ty == INTERGENIC:
            tot["n_intergenic_reads"] += 1
            continue
        if ty == INTRONIC and not flags & INTRONIC_FLAG:
            tot["n_intronic_skipped_reads"] += 1
            continue
        gene = tx_gene[idx] if ty == EXONIC else idx
        tag = parse_tag(nm[r], cb_len, umi_len)
        if tag is None:
            tot["n_untagged_reads"] += 1
            continue
        tot["n_counted_reads"] += 1
        key = (tag[0], gene, tag[1])
        mol[key] = mol.get(key, 0) + 1
    return mol, tot


def add_molecules(a, b):
    out = dict(a)
    for k, v in b.items():
        out[k] = out.get(k, 0) + v
    return out


def add_totals(a, b):
    return {k: a[k] + b[k] for k in TOTAL_NAMES}


def rows(mol, min_umis=1):
    """-> (cells CELL_DT, entries ENTRY_DT, dict(n_molecules, n_barcodes, n_cells_below)) of a fetch"""
    per_bc = {}
    for (bc, gene, umi), n in mol.items():
        per_bc.setdefault(bc, {}).setdefault(gene, []).append(n)
    cells, entries = [], []
    for bc in sorted(per_bc):
        genes = per_bc[bc]
        n_umis = sum(len(v) for v in genes.values())
        if n_umis < min_umis:
            continue
        for g in sorted(genes):
            entries.append((len(cells), g, len(genes[g]), sum(genes[g])))
        cells.append((sum(sum(v) for v in genes.values()), bc, n_umis, len(genes), 0))
    return (np.array(cells, CELL_DT) if cells else np.zeros(0, CELL_DT), np.array(entries, ENTRY_DT) if entries else np.zeros(0, ENTRY_DT),
            dict(n_molecules=len(mol), n_barcodes=len(per_bc), n_cells_below=len(per_bc) - len(cells)))


def pack_rows(cells, entries):
    """the two arrays as the bytes a fetch's buffer holds"""
    return np.ascontiguousarray(cells, CELL_DT).tobytes() + np.ascontiguousarray(entries, ENTRY_DT).tobytes()


def assert_result(res, mol, tot, min_umis=1, what=""):
    """a capi.CellsResult against the molecules and totals"""
    cells, entries, counts = rows(mol, min_umis)
    assert res.totals == tot, (what, res.totals, tot)
    assert (res.n_molecules, res.n_barcodes, res.n_cells_below) == (counts["n_molecules"], counts["n_barcodes"], counts["n_cells_below"]), what
    assert len(res.cells) == len(cells) and len(res.entries) == len(entries), (what, len(res.cells), len(cells), len(res.entries), len(entries))
    for f in CELL_DT.names:
        bad = np.nonzero(res.cells[f] != cells[f])[0]
        assert len(bad) == 0, "%s cell %d %s: got %s expected %s" % (what, bad[0], f, res.cells[bad[0]], cells[bad[0]])
    for f in ENTRY_DT.names:
        bad = np.nonzero(res.entries[f] != entries[f])[0]
        assert len(bad) == 0, "%s entry %d %s: got %s expected %s" % (what, bad[0], f, res.entries[bad[0]], entries[bad[0]])
    assert pack_rows(res.cells, res.entries) == pack_rows(cells, entries), what
    assert res.min_umis == min_umis


def check_invariants(tot, mol):
    assert tot["n_reads"] == sum(tot[k] for k in TOTAL_NAMES[1:])
    assert tot["n_counted_reads"] == sum(mol.values())


def mtx_of(t, cells, entries, cb_len):
    """the driver's three files as text: (cells.mtx, cells.barcodes.tsv, cells.features.tsv)"""
    mtx = ["%%MatrixMarket matrix coordinate integer general\n", "%d %d %d\n" % (len(t["genes"]), len(cells), len(entries))]
    mtx += ["%d %d %d\n" % (int(e["gene"]) + 1, int(e["cell"]) + 1, int(e["n_umis"])) for e in entries]
    barcodes = "".join(unpack(int(c["barcode"]), cb_len) + "\n" for c in cells)
    features = "".join("%s\t%s\tGene Expression\n" % (t["gene_ids"][g], t["gene_names"][g]) for g in range(len(t["genes"])))
    return "".join(mtx), barcodes, features


# ------------------------------------------------------------------ names
def gen_names(n, seed, cb_len=16, umi_len=12, n_barcodes=7, n_umis=5, untagged=0.1):
    """n read names: prefix, '_', a barcode of a pool of n_barcodes, '_', a UMI of a pool of n_umis, a third of them with a
    comment behind a space (which itself ends like a tag of other sequences); a fraction `untagged` of them spoiled in
    turn by an N, a lower-case base, '-' for a '_', a cut that leaves the QNAME one byte short, or no tag at all"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    bcs = [bytes(acgt[rng.integers(0, 4, cb_len)]) for _ in range(n_barcodes)]
    umis = [bytes(acgt[rng.integers(0, 4, umi_len)]) for _ in range(n_umis)]
    # (the barcodes are drawn unevenly: the last ones are rare, so that a min_umis filter removes some and keeps some)
    weights = np.array([4.0 ** -k for k in range(n_barcodes)])
    weights /= weights.sum()
    out = []
    spoil = 0
    for i in range(n):
        bc, umi = bcs[int(rng.choice(n_barcodes, p=weights))], umis[int(rng.integers(0, n_umis))]
        q = b"r%d_" % i + bc + b"_" + umi
        if rng.random() < untagged:
            kind = spoil % 5
            spoil += 1
            if kind == 0:
                q = q[:-1] + b"N"
            elif kind == 1:
                q = q[: len(q) - umi_len - 2] + q[len(q) - umi_len - 2: len(q) - umi_len - 1].lower() + q[len(q) - umi_len - 1:]
            elif kind == 2:
                q = q[: len(q) - umi_len - 1] + b"-" + umi
            elif kind == 3:
                q = q[len(q) - (cb_len + umi_len + 1):]     # one byte shorter than a tag
            else:
                q = b"r%d" % i
        if i % 3 == 0:
            q += b" 1:N:0_" + b"T" * cb_len + b"_" + b"G" * umi_len
        out.append(q)
    return out


# ------------------------------------------------------------------ the tag-parse cases, each with what the contract says of it
def tag_cases(cb_len, umi_len):
    """[(name, tagged)] for lengths cb_len / umi_len: the cases of the contract's first paragraph"""
    bc, umi = (b"ACGTTGCAACGTTGCA" * 2)[:cb_len], (b"TTGACCAGTCAGGTCA" * 2)[:umi_len]
    tag = b"_" + bc + b"_" + umi
    low = lambda s, i: s[:i] + s[i: i + 1].lower() + s[i + 1:]   # noqa: E731
    n_at = lambda s, i: s[:i] + b"N" + s[i + 1:]                 # noqa: E731
    return [
        (tag, True),                                   # the QNAME is exactly the tag: an empty prefix
        (tag[1:], False),                              # one byte shorter
        (b"read7" + tag, True),
        (b"read7" + tag + b" comment", True),
        (b"read7 c" + tag, False),                     # the tag-like tail lies behind the first space
        (b"read7" + tag + b" x" + b"_" + b"A" * cb_len + b"_" + b"C" * umi_len, True),   # ... a comment's is ignored: the QNAME's counts
        (b"x" + b"_" + n_at(bc, 0) + b"_" + umi, False),
        (b"x" + b"_" + bc + b"_" + n_at(umi, umi_len - 1), False),
        (b"x" + b"_" + low(bc, cb_len - 1) + b"_" + umi, False),
        (b"x" + b"_" + bc + b"_" + low(umi, 0), False),
        (b"x" + b"-" + bc + b"_" + umi, False),
        (b"x" + b"_" + bc + b"-" + umi, False),
        (b"", False),
        (b" ", False),
        (b" " + tag, False),                           # an empty QNAME
        (b"plain", False),
        (b"last" + tag, True),                         # (the name that ends the pool)
    ]


# ------------------------------------------------------------------ a view with every class of read
def class_view(t, cb_len, umi_len):
    """-> (offsets, alns, status, names, cigar view parts) over big_gene_tables(): counted exonic and intronic reads on the
    first and the last gene, multi, unmapped, intergenic, failed and untagged reads, reads without alignments between reads
    with them, and the barcodes AAAA... and TTTT... beside a mixed one"""
    n_genes = len(t["genes"])
    bcs = [b"A" * cb_len, b"T" * cb_len, (b"GATTACAGATTACAGA")[:cb_len]]
    umis = [b"C" * umi_len, (b"TGCATGCATGCATGCA")[:umi_len], b"T" * umi_len]
    reads, names, status = [], [], []
    ex = lambda g: dict(ref_id=0, ystart=500 + 105 * g, aln_type=EXONIC, idx=g, cigar=[(50, "M")])       # noqa: E731  (tx g is gene g's)
    intr = lambda g: dict(ref_id=0, ystart=500 + 105 * g, aln_type=INTRONIC, idx=g, cigar=[(50, "M")])   # noqa: E731
    inter = dict(ref_id=1, ystart=77, aln_type=INTERGENIC, idx=0xFFFFFFFF, cigar=[(50, "M")])
    k = 0
    for bc in bcs:
        for g in (0, 1, n_genes - 1, 8191, 8192):
            for umi in umis:
                for rep in range(1 + (k % 3)):
                    reads.append([ex(g)])
                    names.append(b"q%d_" % k + bc + b"_" + umi + (b" c" if k % 2 else b""))
                    status.append(0)
                k += 1
        reads += [[intr(n_genes - 1)], [], [ex(5), ex(6)], [inter], [], [ex(7)], [ex(8)], [ex(9)], [intr(0)]]
        tag = b"_" + bc + b"_" + umis[0]
        names += [b"i" + tag, b"u" + tag, b"m" + tag, b"g" + tag, b"", b"f" + tag, b"plain", b"x" + tag[:-1] + b"N", b"i2" + tag]
        status += [0, 0, 0, 0, 0, -7, 0, 0, 0]
    import quant_common as qc
    offsets, alns, dig, words = qc.make_view(reads)
    return offsets, alns, np.array(status, "<i4"), names, (dig, words)


# ------------------------------------------------------------------ the model program's input and output
def model_input(t, offsets, alns, status, names, name_off, flags, cb_len, umi_len, min_umis):
    """one case as the bytes tests/cpp/cells_model_main.cpp reads"""
    offsets = np.ascontiguousarray(offsets, "<u8")
    alns = np.ascontiguousarray(alns, capi.ALN_DT)
    names = np.ascontiguousarray(names, np.uint8)
    name_off = np.ascontiguousarray(name_off, "<u8")
    head = np.array([len(offsets) - 1, len(alns), len(t["txs"]), len(t["genes"]), 0 if status is None else 1, flags, cb_len, umi_len, min_umis,
                     len(names)], "<u8")
    parts = [head, offsets, alns, np.ascontiguousarray(t["txs"]["gene_idx"], "<u4"), name_off]
    if status is not None:
        parts.append(np.ascontiguousarray(status, "<i4"))
    parts.append(names)
    return b"".join(p.tobytes() for p in parts)


def model_output(out):
    """-> (totals dict, counts dict, cells, entries, molecule rows as [(barcode, gene, umi, reads)])"""
    head = np.frombuffer(out[: 8 * 13], "<u8")
    tot = {k: int(v) for k, v in zip(TOTAL_NAMES, head[:8])}
    n_mol, n_bc, n_below, n_cells, n_entries = (int(x) for x in head[8:13])
    at = 8 * 13
    cells = np.frombuffer(out[at: at + 24 * n_cells], CELL_DT)
    at += 24 * n_cells
    entries = np.frombuffer(out[at: at + 16 * n_entries], ENTRY_DT)
    at += 16 * n_entries
    mols = np.frombuffer(out[at:], "<u4").reshape(-1, 4)
    assert len(mols) == n_mol
    return tot, dict(n_molecules=n_mol, n_barcodes=n_bc, n_cells_below=n_below), cells, entries, [tuple(int(x) for x in m) for m in mols]
