"""-m gpu: the text position in single-suffix entries of the device's k-mer table (thermite_amd/csrc/lut_direct.h).

When the device copy of an index is made, one pass writes TAG | sa[lo] over hi of every table entry with hi - lo == 1;
a seed probe that lands in such a bucket then goes from the entry to the text without reading the suffix array
(kernels_seed.hip, ms_search).  THM_LUT_DIRECT=0 leaves the table plain; bit 6 of thm_debug_set_flags makes the probes
ignore the stored position (bit 7: use it again); thm_debug_seed_direct_stats reports whether the table is tagged, how
many entries the pass rewrote and, with the probes counted, how many full probes took the position from the entry and how
many read the suffix array for a one-suffix bucket.

  * the device table against the host's, at both coordinate widths, on test_ref, chrM and the synthetic text of
    seed_direct_common.py; plain under THM_LUT_DIRECT=0 (a fresh child process);
  * check_smems and check_align against the oracle for every case of seed_direct_common.py with the position used and
    ignored, at both widths, and once under THM_LUT_DIRECT=0;
  * the counts say which path ran, and SMEMs, records, op bytes and counters are equal either way."""
import os
import subprocess
import sys

import numpy as np
import pytest

from thermite_amd import capi, refdata

import seed_direct_common as sd
from oracle import pyoracle as orc

from gpu_common import World, assert_counters_match, check_align, check_smems

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")
CHILD = os.path.join(ROOT, "tests", "seed_direct_child.py")
CHILD_LIMIT = 120   # seconds; the child takes a few (interpreter start, index of 100 kilobases, two batches of ~700 reads)

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def reference(name):
    def make():
        if name == "synthetic":
            return sd.tables()
        stem = {"test_ref": "test_ref", "chrM": "GRCh38-2020-A-chrM"}[name]
        return refdata.load_reference(os.path.join(DATA, stem + ".fasta"), os.path.join(DATA, stem + ".gtf"))
    return _once(("ref", name), make)


class SynthWorld(World):
    """a World over the synthetic text, indexed with THM_KT = 8"""

    def __init__(self, wide):
        self.t = sd.tables()
        self.ix = sd.make_index(self.t, wide)
        self.oix = orc.Index(self.t, sa=self.ix.suffix_array())
        self._a = None


def world(wide):
    return _once(("world", wide), lambda: SynthWorld(wide))


def oracle_alignments(name):
    def make():
        bases, off = sd.case_batch(name)
        return world(False).oix.align_batch(bases, off, sd.OPTS, n_threads=8)
    return _once(("oracle", name), make)


def expected_device_table(host, sa, wide):
    """the host table with TAG | sa[lo] in hi of every entry with hi - lo == 1; the number of such entries"""
    tag = np.uint64(1) << np.uint64(63 if wide else 31)
    want = host.astype(np.uint64)
    single = (want[:, 1] - want[:, 0]) == 1
    want[single, 1] = tag | sa.astype(np.uint64)[want[single, 0].astype(np.int64)]
    return want.astype(host.dtype), int(single.sum())


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
@pytest.mark.parametrize("name", ["test_ref", "chrM", "synthetic"])
def test_device_table_against_host(name, wide):
    t = reference(name)
    ix = sd.make_index(t, wide) if name == "synthetic" else capi.Index(t, wide=wide)
    host, sa = ix.debug_host_lut(), ix.suffix_array()
    want, n_single = expected_device_table(host, sa, wide)
    assert n_single > 0 and n_single < len(host)
    a = capi.Aligner(ix, capi.CI_OPTS)
    got = a.debug_fetch_lut(host)
    tagged, n_tagged, _, _ = a.debug_seed_direct_stats()
    b = capi.Aligner(ix, capi.CI_OPTS)     # a second aligner shares the device copy: the pass does not run twice
    again = b.debug_fetch_lut(host)
    stats_b = b.debug_seed_direct_stats()
    b.close()
    a.close()
    assert ix.check_lut() and np.array_equal(ix.debug_host_lut(), host)   # the host table is untouched
    ix.close()
    assert tagged == 1 and n_tagged == n_single, (tagged, n_tagged, n_single)
    assert got.dtype == want.dtype and np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0][:10]
    assert np.array_equal(again, want) and stats_b[:2] == (1, n_single)


# ------------------------------------------------------------------ parity with the oracle
CASE_NAMES = ["absent", "bucket_2", "bucket_60", "bucket_8", "bucket_9", "contig_end", "n_in_read", "one_exact", "one_sub_anywhere",
              "one_tail_sub", "short"]   # (written out: building the cases needs an index, collecting the tests must not)


def test_the_cases_sit_where_they_say():
    text, sa, lut, size = sd.host_view()
    c = sd.cases()
    code_of = {int(b): i for i, b in enumerate(sd.ACGT)}

    def bucket(read):
        code = 0
        for b in read[: sd.KT]:
            code = code * 4 + code_of[int(b)]
        return int(lut[code, 1] - lut[code, 0])
    assert all(bucket(r) == 1 for n in ("one_tail_sub", "short") for r in c[n])
    assert sum(bucket(r) == 1 for r in c["one_sub_anywhere"]) >= 80   # (all but the substitutions inside the kt-mer)
    assert sum(bucket(r) == 1 for r in c["one_exact"]) >= 12   # (a reverse complement starts with another kt-mer)
    assert all(bucket(r) == 2 for r in c["bucket_2"][::4]) and all(bucket(r) == 8 for r in c["bucket_8"][::4])
    assert all(bucket(r) == 9 for r in c["bucket_9"][::4]) and all(bucket(r) >= 60 for r in c["bucket_60"][::4])
    assert all(bucket(r) == 0 for r in c["absent"])
    assert all(bucket(r) == 1 for r in c["contig_end"])
    lens = {len(r) for r in c["short"]}
    assert lens == {sd.K - 1, sd.K, sd.K + 1}
    tails = {len(r) - sd.KT for r in c["one_exact"]}
    assert {80, 81, 83} <= tails   # two round trips of eight words with 16, 17 and 19 bytes in the second


class FlagWorld:
    """what check_smems and check_align use of a World; its aligners use or ignore the stored positions, count their seed
    probes and leave the counts in .stats when the check closes them"""

    def __init__(self, w, direct):
        self.t, self.ix, self.oix = w.t, w.ix, w.oix
        self.direct = direct
        self.stats = []

    def aligner(self, opts):
        fw = self

        class A(capi.Aligner):
            def close(self):
                if getattr(self, "h", None):
                    fw.stats.append(self.debug_seed_direct_stats())
                super().close()
        a = A(self.ix, opts)
        a.debug_set_flags(seed_stats=True, seed_direct=self.direct)
        return a


@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_parity(name, wide):
    bases, off = sd.case_batch(name)
    ref = oracle_alignments(name)
    for direct in (True, False):
        fw = FlagWorld(world(wide), direct)
        check_smems(fw, bases, off, sd.K)
        check_align(fw, bases, off, sd.OPTS, ref=ref)
        assert len(fw.stats) == 3, fw.stats   # smems_batch, align_batch with and without the problem-parallel path
        print(name, "wide" if wide else "narrow", "direct" if direct else "via sa", fw.stats)
        for tagged, n_tagged, used, via_sa in fw.stats:
            assert tagged == 1 and n_tagged > 0
            assert (via_sa == 0) if direct else (used == 0), fw.stats
    # k = kt: the table entry alone is a seed
    fw = FlagWorld(world(wide), True)
    check_smems(fw, bases, off, sd.KT)


def test_case_names_are_complete():
    assert sorted(sd.cases()) == CASE_NAMES


# ------------------------------------------------------------------ which path ran; equal results either way
def _assert_same_results(x, y):
    for f in ("smem_off", "smem_mems", "offsets", "alns", "ops", "counters"):
        assert np.array_equal(x[f], y[f]), f
    assert np.array_equal(x["stats"], y["stats"]) and np.array_equal(x["smem_stats"], y["smem_stats"])   # the same probes


@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
def test_the_path_is_taken(wide):
    w = world(wide)
    bases, off = sd.case_batch("all")
    on = sd.device_run(w.ix, bases, off, seed_direct=True)
    off_ = sd.device_run(w.ix, bases, off, seed_direct=False)
    back = sd.device_run(w.ix, bases, off, seed_direct=True)
    print("direct", on["direct"], on["smem_direct"], "ignored", off_["direct"], off_["smem_direct"], "probes", on["stats"])
    for r in (on, back):
        for key in ("direct", "smem_direct"):
            assert r[key][0] == 1 and r[key][1] > 0 and r[key][2] > 0 and r[key][3] == 0, r[key]
    for key in ("direct", "smem_direct"):
        assert off_[key][0] == 1 and off_[key][2] == 0 and off_[key][3] > 0, off_[key]
        assert off_[key][3] == on[key][2]      # the same probes, by the other road
        assert on[key][2] <= on["stats" if key == "direct" else "smem_stats"][1]   # they are full probes
    assert np.array_equal(on["lut"], off_["lut"])   # bit 6 leaves the table tagged
    _assert_same_results(on, off_)
    _assert_same_results(on, back)
    ref = oracle_alignments("all")
    assert np.array_equal(on["offsets"], ref.offsets) and np.array_equal(on["alns"], ref.alns) and np.array_equal(on["ops"], ref.ops)
    assert_counters_match(on["counters"], ref.counters, "direct")


@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
def test_plain_table_under_the_knob(tmp_path, wide):
    """THM_LUT_DIRECT=0 in a fresh process: nothing is tagged, every one-suffix probe reads the suffix array, and the
    results are the oracle's and the tagged table's"""
    out = str(tmp_path / "out.npz")
    cmd = [sys.executable, CHILD, "64" if wide else "32", out]
    p = subprocess.run(cmd, env=dict(os.environ, THM_LUT_DIRECT="0"), timeout=CHILD_LIMIT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True)
    assert p.returncode == 0, p.stderr[-4000:]
    with np.load(out) as z:
        plain = {k: z[k] for k in z.files}
    w = world(wide)
    host = w.ix.debug_host_lut()
    assert np.array_equal(plain["lut"], host)            # bit-identical to the host's table
    for key in ("direct", "smem_direct"):
        assert plain[key][0] == 0 and plain[key][1] == 0 and plain[key][2] == 0 and plain[key][3] > 0, plain[key]
    bases, off = sd.case_batch("all")
    ref = oracle_alignments("all")
    assert np.array_equal(plain["offsets"], ref.offsets) and np.array_equal(plain["alns"], ref.alns) and np.array_equal(plain["ops"], ref.ops)
    assert_counters_match(plain["counters"], ref.counters, "plain")
    r = w.oix.all_smems(bases, off, sd.K)
    assert np.array_equal(plain["smem_off"], r.offsets)
    for f in ("ref_idx", "query_idx", "len"):
        assert np.array_equal(plain["smem_mems"][f], r.mems[f]), f
    on = sd.device_run(w.ix, bases, off)
    _assert_same_results(on, plain)
    assert plain["direct"][3] == on["direct"][2]
