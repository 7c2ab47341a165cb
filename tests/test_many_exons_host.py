"""CPU: the inputs of tests/test_gpu_many_exons.py, pinned with the oracle alone.  The register-resident extend kernels
keep at most 64 intron markers per alignment (FAST_MAX_YCLIPS, extend_plan.h) and hand a read that needs more to the
any-width kernel; the GPU tests of that hand-over mean something only if their reads have alignments on both sides of the
limit.  That is asserted here, where no device is involved."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from thermite_amd import capi

from gpu_common import MARKER_LIMIT, MICRO_OPTS, exonic_yclip_counts, micro_exon_reads, micro_exon_reference


@pytest.fixture(scope="module")
def micro():
    t = micro_exon_reference()
    return t, orc.Index(t, sa=capi.build_suffix_array(t["text"]))


def test_reference_arms_the_retry(micro):
    t, _ = micro
    assert int(t["txs"]["n_exons"].max()) > MARKER_LIMIT + 1  # pipeline.hip: retry_possible
    assert len(t["_micro"]) >= 4 and {m["strand"] for m in t["_micro"]} == {True, False}
    plain = micro_exon_reference(with_micro=False)
    assert int(plain["txs"]["n_exons"].max()) <= MARKER_LIMIT + 1
    assert np.array_equal(plain["text"], t["text"])
    n = len(plain["txs"])
    assert n == len(t["txs"]) - len(t["_micro"]) and np.array_equal(plain["exons"], t["exons"][: len(plain["exons"])])


@pytest.mark.parametrize("mutated", [False, True], ids=["exact", "mutated"])
@pytest.mark.parametrize("opts", [MICRO_OPTS, dict(MICRO_OPTS, intron_mode=False, multimap_score_range=3)], ids=["intron", "no_intron_mm3"])
def test_read_sets_reach_both_sides_of_the_marker_limit(micro, mutated, opts):
    t, oix = micro
    bases, off, _ = micro_exon_reads(t, mutated=mutated)
    lens = np.diff(off.astype(np.int64))
    for L in (91, 150, 200, 250):
        assert (np.abs(lens - L) <= 3).sum() >= 20
    r = oix.align_batch(bases, off, opts, n_threads=4)
    assert r.counters[15] == 0, "oracle saw reads where the reference would panic"
    y = exonic_yclip_counts(r)
    assert (y == MARKER_LIMIT).sum() >= 5
    assert (y == MARKER_LIMIT + 1).sum() >= 5
    assert (y > MARKER_LIMIT).sum() >= 50
    assert ((y >= 1) & (y <= MARKER_LIMIT)).sum() >= 50
    if mutated:  # the edits reach the alignments: ops other than Match and Yclip
        exonic = np.nonzero(r.alns["aln_type"] == 0)[0]
        edited = 0
        for i in exonic:
            a = r.alns[i]
            ops = orc.decode_ops(r.ops[int(a["ops_off"]): int(a["ops_off"]) + int(a["ops_len"])])
            edited += any(o in ("Subst", "Ins", "Del") for o in ops)
        assert edited >= 100
