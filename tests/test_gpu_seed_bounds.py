"""-m gpu: grid-cell positions of the seed stage decided from the bounds of the two grid probes (thermite_amd/csrc/seed_bounds.h).

A probe knows the match end of its position also where the match is shorter than k (exactly, or -- after an empty bucket
of the k-mer table -- to within kt), and the match end never decreases along the read.  So an inner position of a grid
cell needs no probe where the right grid point's bound leaves no room for a match of k bases, or where both bounds
agree.  Bit 16 of thm_debug_set_flags turns the rule off (bit 17: on again); it does not hang on bit 2, the table-entry
shortcut, and neither changes which positions the other probes.

Every case goes through gpu_common.check_smems and check_align against the oracle, at 32- and 64-bit coordinates, with
the rule on and off.  The probes the kernels count (thm_debug_seed_stats: decided + full) must be what the host model of
tests/cpp/seed_bounds_main.cpp counts for the same text and reads, in both settings and with bit 2 set and clear, and
fewer with the rule on wherever a read has one substitution."""
import numpy as np
import pytest

from thermite_amd import capi

import seed_bounds_common as sb
from gpu_common import World, check_align, check_smems

pytestmark = pytest.mark.gpu


def world(wide):
    def make():
        w = World.__new__(World)
        w.t = sb.tables()
        w.ix = sb.make_index(w.t, wide)
        assert w.ix.coord_bytes == (8 if wide else 4)
        from oracle import pyoracle as orc
        w.oix = orc.Index(w.t, sa=w.ix.suffix_array())
        w._a = None
        return w
    return sb.once(("world", wide), make)


class _CountingAligner(capi.Aligner):
    sink = None

    def close(self):
        if getattr(self, "h", None) and self.sink is not None:
            self.sink.append(sum(self.debug_seed_stats()))   # decided + full of the aligner's one batch
        super().close()


class FlagWorld:
    """what check_smems and check_align use of a World; its aligners have the rule and the shortcut as given, count
    their seed probes and leave decided + full in .probes when the check closes them"""

    def __init__(self, w, bounds, infer):
        self.t, self.ix, self.oix = w.t, w.ix, w.oix
        self.bounds, self.infer = bounds, infer
        self.probes = []

    def aligner(self, opts):
        a = _CountingAligner(self.ix, opts)
        a.sink = self.probes
        a.debug_set_flags(seed_bounds=self.bounds, seed_infer=self.infer, seed_stats=True)
        return a


def oracle_alignments(name):
    """the oracle's alignments of a case: once, for both widths and all settings"""
    def make():
        bases, off, k = sb.case(name)
        return world(False).oix.align_batch(bases, off, dict(sb.OPTS, min_seed_len=k), n_threads=8)
    return sb.once(("oracle", name), make)


def test_the_cases_are_what_they_claim():
    t = sb.tables()
    main = t["_main"]
    assert np.array_equal(main[sb.DUP_A: sb.DUP_A + sb.DUP_LEN], main[sb.DUP_B: sb.DUP_B + sb.DUP_LEN])
    assert main[sb.DUP_A + sb.DUP_LEN] != main[sb.DUP_B + sb.DUP_LEN] and main[sb.DUP_A - 1] != main[sb.DUP_B - 1]
    lens = np.diff(sb.case("one_long_among_short")[1].astype(np.int64))
    assert (lens == 300).sum() == 1 and (lens == 91).sum() == len(lens) - 1
    for name, L in (("one_sub_L29", 29), ("one_sub_L35", 35), ("length_k", sb.K), ("length_k_plus_1", sb.K + 1)):
        lens = np.diff(sb.case(name)[1].astype(np.int64))
        assert (lens == L).all()
        assert (L - sb.K) % 8 != 0 or L - sb.K < 8   # the last cell is short, or there is none
    for name in sb.CASES:
        assert len(sb.case(name)[1]) - 1 <= 400, name
    for name in sb.ONE_SUB:
        off, on = sb.host_probe_counts(name)
        assert on < off, (name, off, on)


@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
@pytest.mark.parametrize("name", sorted(sb.CASES))
def test_seed_bounds(name, wide):
    bases, off, k = sb.case(name)
    opts = dict(sb.OPTS, min_seed_len=k)
    ref = oracle_alignments(name)
    host = dict(zip((False, True), sb.host_probe_counts(name)))
    got = {}
    for bounds in (True, False):
        fw = FlagWorld(world(wide), bounds, True)
        check_smems(fw, bases, off, k)
        check_align(fw, bases, off, opts, ref=ref)
        assert len(fw.probes) == 3, fw.probes   # smems_batch, align_batch with and without the problem-parallel path
        print(name, "wide" if wide else "narrow", "bounds" if bounds else "whole cells", fw.probes, "host", host[bounds])
        assert fw.probes == [host[bounds]] * 3, (fw.probes, host)
        got[bounds] = fw.probes[0]
        # the table-entry shortcut (bit 2) off: the same positions are probed
        fw = FlagWorld(world(wide), bounds, False)
        check_smems(fw, bases, off, k)
        assert fw.probes == [host[bounds]], (fw.probes, host)
    if name in sb.ONE_SUB:
        assert got[True] < got[False], got
    else:
        assert got[True] <= got[False], got
