"""Reference, reads and helpers of tests/test_gpu_seed_bounds.py, and the build of tests/cpp/seed_bounds_main.cpp that
tests/test_seed_bounds_host.py shares with it.

One text of 36 kilobases in two contigs (an N run, a 60-base stretch that occurs twice), indexed with THM_KT = 8.  The
host program models which positions the seed kernels probe with the cell rule of thermite_amd/csrc/seed_bounds.h on and
off; `host_probe_counts` hands it a case (the index text, the reads, k, kt) and returns both counts, which
thm_debug_seed_stats must report as decided + full."""
import os
import struct
import subprocess
import tempfile

import numpy as np

from thermite_amd import capi, refdata, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KT = 8
K = 20
ACGT = np.frombuffer(b"ACGT", np.uint8)
MAIN_LEN, SECOND_LEN = 30000, 6000
DUP_A, DUP_B, DUP_LEN = 5000, 9000, 60       # main[DUP_B : DUP_B + 60] is a copy of main[DUP_A : DUP_A + 60]
N_RUN = (15000, 15200)                       # main[15000:15200] is N
OPTS = dict(capi.CI_OPTS)

_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ------------------------------------------------------------------ the host program
def build_host_program(out_dir, sanitizers=False):
    exe = os.path.join(str(out_dir), "seed_bounds_main" + ("_san" if sanitizers else ""))
    extra = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitizers else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + extra +
                          ["-I" + os.path.join(ROOT, "thermite_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "seed_bounds_main.cpp"), "-o", exe])
    return exe


def host_program():
    def make():
        d = tempfile.mkdtemp(prefix="seed_bounds_")
        return build_host_program(d)
    return once("exe", make)


def write_batch(path, text, bases, off, k, kt):
    off = np.asarray(off, "<u8")
    with open(path, "wb") as f:
        f.write(b"SBD1" + struct.pack("<IIQQ", k, kt, len(text), len(off) - 1))
        f.write(off.tobytes())
        f.write(np.ascontiguousarray(text, np.uint8).tobytes())
        f.write(np.ascontiguousarray(bases, np.uint8)[: int(off[-1])].tobytes())


def host_probe_counts(name):
    """(probes with the rule off, with the rule on) of a case, from the host program; once per case"""
    def make():
        bases, off, k = case(name)
        path = os.path.join(os.path.dirname(host_program()), name + ".batch")
        write_batch(path, tables()["text"], bases, off, k, KT)
        out = subprocess.run([host_program(), "--file", path], check=True, capture_output=True, text=True).stdout.split()
        os.remove(path)
        assert out[0] == "probes", out
        return int(out[1]), int(out[2])
    return once(("host", name), make)


# ------------------------------------------------------------------ the reference
def other(*avoid):
    return int([b for b in ACGT if int(b) not in [int(a) for a in avoid]][0])


def _make_tables():
    rng = np.random.Generator(np.random.PCG64(0xB0D5))
    main = ACGT[rng.integers(0, 4, MAIN_LEN)].copy()
    main[DUP_B: DUP_B + DUP_LEN] = main[DUP_A: DUP_A + DUP_LEN]
    main[DUP_B - 1] = other(main[DUP_A - 1])               # the copies differ in front ...
    main[DUP_B + DUP_LEN] = other(main[DUP_A + DUP_LEN])   # ... and behind
    main[N_RUN[0]: N_RUN[1]] = ord("N")
    second = ACGT[rng.integers(0, 4, SECOND_LEN)].copy()
    genes, txs = synth.synth_annotation(rng, "main", MAIN_LEN, 100, 4)
    t = refdata.build_tables([("main", main), ("second", second)], genes, txs)
    t["_main"], t["_second"] = main, second
    return t


def tables():
    return once("tables", _make_tables)


def make_index(t, wide):
    old = os.environ.get("THM_KT")
    os.environ["THM_KT"] = str(KT)   # read when the index is created
    try:
        return capi.Index(t, wide=wide)
    finally:
        if old is None:
            del os.environ["THM_KT"]
        else:
            os.environ["THM_KT"] = old


def sub(read, p):
    r = np.array(read, np.uint8)
    r[p] = other(r[p])
    return r


def window(s, L, contig="_main"):
    return tables()[contig][s: s + L].copy()


# ------------------------------------------------------------------ the cases: name -> (reads, k)
def _one_sub(L, k=K, step=1):
    w, v = window(2000, L), refdata.revcomp(window(21011, L))
    return [sub(w, p) for p in range(0, L, step)] + [sub(v, p) for p in range(0, L, step)], k


def _two_subs():
    w = window(3000, 91)
    reads = []
    for gap in (K - 1, K, K + 1, K + 9):
        reads += [sub(sub(w, p), p + gap) for p in range(0, 91 - gap)]
    return reads, K


def _duplicate():
    """reads that run through one copy of the duplicated stretch into its flank, with a substitution in front of, inside
    and shortly behind the stretch: a grid point of the stretch whose match along the read's own locus is cut short
    still has the other copy to match"""
    reads = []
    for at in (DUP_A, DUP_B):
        for s in range(0, 40, 2):
            r = window(at + s - 20, 91)
            end = 20 + DUP_LEN - s       # read position of the first base behind the stretch
            reads += [r, sub(r, end + 3), sub(r, end - 5), sub(r, 10), sub(sub(r, 10), end + 3)]
    return reads, K


def _empty_bucket():
    w = window(4500, 91)
    return [sub(w, gp + j) for gp in range(8, 72, 8) for j in range(KT)], K


def _n_and_contig_end():
    rng = np.random.Generator(np.random.PCG64(0xE2D))
    reads = []
    for n in (30, 40, 47, 48, 49, 60):
        tail = ACGT[rng.integers(0, 4, 91 - n)]
        reads.append(np.concatenate([window(SECOND_LEN - n, n, "_second"), tail]))   # the match stops at '$'
        reads.append(np.concatenate([window(MAIN_LEN - n, n), tail]))
        reads.append(np.concatenate([window(N_RUN[0] - n, n), tail]))                # ... at the N run
        reads.append(window(N_RUN[0] - n, 91))                                       # N against N: it goes on
        reads.append(refdata.revcomp(np.concatenate([tail, window(0, n, "_second")])))  # the other strand's contig end
    w = window(4000, 91)
    for p in (0, 7, 8, 33, 45, 70, 90):
        for c in (b"N", b"n", b"X", b"*", b"\x00", b"$"):
            r = w.copy()
            r[p] = c[0]
            reads.append(r)
    r = w.copy()
    r[40:44] = ord("N")
    reads.append(r)
    return reads, K


def _indels():
    reads = []
    w = window(12000, 92)
    for p in range(4, 88, 2):
        reads.append(np.concatenate([w[:p], [other(w[p - 1], w[p])], w[p: 90]]).astype(np.uint8))   # one inserted base
        reads.append(np.concatenate([w[:p], w[p + 1:]]).astype(np.uint8))                            # one deleted base
    return reads, K


def _one_long():
    reads = [sub(window(2000 + 97 * i, 91), (7 * i) % 91) for i in range(40)]
    w = window(10300, 300)
    for p in range(17, 300, 61):
        w = sub(w, p)
    reads.insert(len(reads) // 2, w)
    return reads, K


CASES = {
    "one_sub_L91": lambda: _one_sub(91),
    "one_sub_L29": lambda: _one_sub(29),
    "one_sub_L35": lambda: _one_sub(35),
    "length_k": lambda: _one_sub(K),
    "length_k_plus_1": lambda: _one_sub(K + 1),
    "two_subs": _two_subs,
    "duplicate": _duplicate,
    "empty_bucket": _empty_bucket,
    "k40": lambda: _one_sub(140, 40, 2),
    "k_is_kt": lambda: _one_sub(50, KT),
    "k_below_kt": lambda: _one_sub(40, KT - 2),
    "n_and_contig_end": _n_and_contig_end,
    "indels": _indels,
    "one_long_among_short": _one_long,
}
ONE_SUB = ("one_sub_L91", "one_sub_L29", "one_sub_L35")   # the rule must remove probes here


def case(name):
    def make():
        reads, k = CASES[name]()
        bases, off = refdata.pack_reads([np.asarray(r, np.uint8) for r in reads])
        return bases, off, k
    return once(("case", name), make)
