"""The finisher's decision (thermite_amd/csrc/smem_finish.h) on the host: tests/cpp/smem_finish_main.cpp runs the header
over seeded batches and, for every read it does not leave, its alignment record, op bytes and counter increments must equal
the CPU oracle's.  Nothing is claimed for a read it leaves -- but the cases that must be left are, and the cases that can be
finished are not all left (the counts are asserted, so no case passes with the rules idle)."""
import numpy as np
import pytest

import gpu_common as gc
import smem_finish_common as sf
from thermite_amd import capi, refdata, synth

L = sf.L0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sf.host_program(tmp_path_factory.mktemp("smem_finish"))


@pytest.fixture(scope="module")
def syn():
    return gc.World(synth.synth_reference(length=300_000))


@pytest.fixture(scope="module")
def planted():
    t, info = sf.planted_reference()
    return gc.World(t), info


def _check(exe, w, opts, reads, tmp_path, **kw):
    bases, off = refdata.pack_reads(reads)
    out, half = sf.run_host(exe, w, opts, bases, off, tmp_path, **kw)
    sf.assert_host_matches_oracle(w, opts, bases, off, out, half)
    return out


@pytest.mark.parametrize("opts", [capi.CI_OPTS, capi.DEFAULT_OPTS], ids=["ci", "default"])
def test_exact_and_substituted_reads_against_the_oracle(exe, syn, opts, tmp_path):
    rng = np.random.default_rng(11)
    out = _check(exe, syn, opts, sf.exact_reads(syn.t, rng), tmp_path, tag="e")
    e_done, e_left, _, _ = sf.finished_counts(out)
    assert e_done >= 40 and e_left >= 4, sf.finished_counts(out)          # inside exons / one base over their ends
    # (an exon lies on one copy of the contig: a reverse-complemented read is unspliced and, without intron mode, not accepted)
    assert (out["accepted"][out["what"] == 1] == 1).sum() >= 10
    if not opts["intron_mode"]:
        assert ((out["what"] == 1) & (out["accepted"] == 0)).sum() >= 10  # unspliced reads are not accepted
    out = _check(exe, syn, opts, sf.subst_reads(syn.t, rng), tmp_path, tag="s")
    _, _, s_done, s_left = sf.finished_counts(out)
    assert s_done >= 100 and s_left >= 10, sf.finished_counts(out)        # a flank that leaves the exon is left


def test_reads_drawn_as_the_benchmark_draws_them(exe, syn, tmp_path):
    bases, off, _ = synth.simulate_reads(syn.t, 3000, L, sub_rate=0.01, indel_rate=0.001, stream=100)
    out, half = sf.run_host(exe, syn, capi.CI_OPTS, bases, off, tmp_path)
    n = sf.assert_host_matches_oracle(syn, capi.CI_OPTS, bases, off, out, half, per_read=32)
    e_done, _, s_done, _ = sf.finished_counts(out)
    assert e_done >= 300 and s_done >= 150 and n == e_done + s_done, sf.finished_counts(out)


def test_each_class_alone(exe, syn, tmp_path):
    bases, off, _ = synth.simulate_reads(syn.t, 800, L, sub_rate=0.01, indel_rate=0.001, stream=101)
    both, _ = sf.run_host(exe, syn, capi.CI_OPTS, bases, off, tmp_path)
    for cls, idx in ((sf.CLASS_E, (0, 1)), (sf.CLASS_S, (2, 3))):
        one, half = sf.run_host(exe, syn, capi.CI_OPTS, bases, off, tmp_path, classes=cls)
        c, cb = sf.finished_counts(one), sf.finished_counts(both)
        assert all(c[k] == (cb[k] if k in idx else 0) for k in range(4)), (c, cb)
        sf.assert_host_matches_oracle(syn, capi.CI_OPTS, bases, off, one, half, per_read=8)


@pytest.mark.parametrize("opts", [
    dict(capi.CI_OPTS, min_aln_score=L + 5),            # no read can reach the threshold: band 0, nothing accepted
    dict(capi.CI_OPTS, min_aln_score=L - 1),            # an exact read passes, one substitution does not
    dict(capi.CI_OPTS, multimap_score_range=0),
    dict(capi.DEFAULT_OPTS, multimap_score_range=3),
], ids=["score_above_L", "score_L_minus_1", "range0", "range3"])
def test_thresholds_and_ranges(exe, syn, opts, tmp_path):
    rng = np.random.default_rng(12)
    reads = sf.exact_reads(syn.t, rng, n_exons=8) + sf.subst_reads(syn.t, rng, n_exons=4)
    out = _check(exe, syn, opts, reads, tmp_path)
    assert (out["what"] == 1).sum() >= 20 or opts["min_aln_score"] > L - 2, sf.finished_counts(out)
    if opts["min_aln_score"] > L:
        assert out["accepted"].sum() == 0


def test_micro_exon_reference(exe, tmp_path):
    w = gc.World(gc.micro_exon_reference())
    rng = np.random.default_rng(13)
    reads = sf.exact_reads(w.t, rng) + sf.subst_reads(w.t, rng, n_exons=6)
    out = _check(exe, w, gc.MICRO_OPTS, reads, tmp_path)
    e_done, _, s_done, _ = sf.finished_counts(out)
    assert e_done >= 20 and s_done >= 20, sf.finished_counts(out)
    # the contig's first and last bases (no N run here): exact reads there are finished, on both copies
    fwd = sf.forward(w.t)
    ends = [fwd[:L], fwd[-L:], refdata.revcomp(fwd[:L]), refdata.revcomp(fwd[-L:])]
    out = _check(exe, w, gc.MICRO_OPTS, ends, tmp_path, tag="ends")
    assert (out["what"] == 1).all() and (out["accepted"] == 1).all(), out


@pytest.mark.parametrize("wide", [False, True], ids=["u32", "u64"])
def test_planted_cases(exe, wide, tmp_path):
    t, info = sf.planted_reference()
    w = gc.World(t, wide=wide)
    rng = np.random.default_rng(14)
    fwd = sf.forward(t)
    # must be left: repeat, two diagonals, indels, N, shorter than k, one repeated base, two-letter repeat
    reads = sf.must_leave_reads(t, info, rng)
    out = _check(exe, w, capi.CI_OPTS, reads, tmp_path, tag="leave")
    left = out["what"] == 0
    assert left[:9].all() and left[len(reads) // 2: len(reads) // 2 + 9].all(), out["what"]
    # an exon that a shorter exon of another isoform overlaps: reads inside the long one, on and off the short one
    a, b, c, d = info["overlap"]
    reads = [fwd[s: s + L] for s in range(a, b - L + 1, 7)]
    out = _check(exe, w, capi.DEFAULT_OPTS, reads, tmp_path, tag="overlap")
    e_done, e_left, _, _ = sf.finished_counts(out)
    assert e_done >= 5 and e_done + e_left == len(reads), sf.finished_counts(out)
    subs = [sf.substitute(r, p, rng) for r in reads for p in (20, 45, L - 21)]
    out = _check(exe, w, capi.DEFAULT_OPTS, subs, tmp_path, tag="overlap_s")
    assert sf.finished_counts(out)[2] >= 5
    # the '-' strand gene, both orientations, flush with the exon's ends
    m0, m1 = info["minus"]
    reads = sf.both_strands([fwd[s: s + L] for s in (m0, m0 + 1, m1 - L, m1 - L - 1, m0 - 1, m1 - L + 1)] * 2)
    reads += [sf.substitute(r, 45, rng) for r in reads]
    out = _check(exe, w, capi.DEFAULT_OPTS, reads, tmp_path, tag="minus")
    assert (out["what"] == 1).sum() >= 12 and (out["accepted"] == 1).sum() >= 6, out[["what", "accepted"]]


def test_same_length_flanks_pin_the_hit_order(exe, syn, tmp_path):
    """p = 45 in a read of 91 bases: both SMEMs have 45 bases, the hit order is the tie rule's"""
    rng = np.random.default_rng(15)
    reads = sf.subst_reads(syn.t, rng, n_exons=10, ps=[45])
    out = _check(exe, syn, capi.CI_OPTS, reads, tmp_path)
    assert sf.finished_counts(out)[2] >= 20


def test_mixed_lengths_and_the_slow_class(exe, syn, tmp_path):
    rng = np.random.default_rng(16)
    fwd = sf.forward(syn.t)
    ex = max(sf.exons_forward(syn.t), key=lambda e: e[1] - e[0])
    reads = [fwd[ex[0]: ex[0] + n] for n in (30, 60, 91, 120, 150, min(ex[1] - ex[0], 300))]
    reads += [sf.substitute(r, len(r) // 2, rng) for r in reads]
    g0 = int(syn.t["refs"][0]["len"]) - 3000
    reads.append(fwd[g0: g0 + 1500])  # band beyond four cells per lane under the CI options: the slow class
    out = _check(exe, syn, capi.CI_OPTS, reads, tmp_path)
    assert out["what"][-1] == 0 and (out["what"][:-1] == 1).sum() >= 8, out["what"]


def test_with_host_sanitizers(syn, tmp_path):
    exe = sf.host_program(tmp_path, sanitizers=True)
    rng = np.random.default_rng(17)
    reads = sf.exact_reads(syn.t, rng, n_exons=6) + sf.subst_reads(syn.t, rng, n_exons=3)
    out = _check(exe, syn, capi.CI_OPTS, reads, tmp_path)
    assert (out["what"] == 1).sum() >= 20
