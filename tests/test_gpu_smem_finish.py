"""The finisher on the device (thermite_amd/csrc/kernels_finish.hip): every case is checked with gpu_common.check_align --
records, op streams and counters against the CPU oracle -- and once more with each class switched off; the counts of
finished and left reads must equal those of the host program over the same header (tests/cpp/smem_finish_main.cpp), so no
case passes with the finisher idle.  The cases are those of tests/test_smem_finish_host.py."""
import numpy as np
import pytest

import gpu_common as gc
import smem_finish_common as sf
from thermite_amd import capi, refdata, synth

pytestmark = pytest.mark.gpu
L = sf.L0
_worlds = {}


def world(name):
    if name not in _worlds:
        if name == "syn":
            _worlds[name] = (gc.World(synth.synth_reference(length=300_000)), None)
        elif name == "micro":
            _worlds[name] = (gc.World(gc.micro_exon_reference()), None)
        elif name in ("planted", "planted64"):
            t, info = sf.planted_reference()
            _worlds[name] = (gc.World(t, wide=name.endswith("64")), info)
        elif name == "heavy":
            t, pos = synth.heavy_repeat_reference(length=600_000, copies=400, n_genes=8)
            _worlds[name] = (gc.World(t), pos)
    return _worlds[name]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sf.host_program(tmp_path_factory.mktemp("smem_finish_gpu"))


check = sf.check_device


def test_exact_reads(exe, tmp_path):
    w, _ = world("syn")
    for k, opts in enumerate((capi.CI_OPTS, capi.DEFAULT_OPTS)):
        c = check(exe, w, opts, sf.exact_reads(w.t, np.random.default_rng(11)), tmp_path)
        assert c[0] >= 40 and c[1] >= 4, c


def test_substituted_reads(exe, tmp_path):
    w, _ = world("syn")
    for opts in (capi.CI_OPTS, capi.DEFAULT_OPTS, dict(capi.CI_OPTS, multimap_score_range=0)):
        c = check(exe, w, opts, sf.subst_reads(w.t, np.random.default_rng(21)), tmp_path)
        assert c[2] >= 100 and c[3] >= 10, c
    c = check(exe, w, capi.CI_OPTS, sf.subst_reads(w.t, np.random.default_rng(15), n_exons=10, ps=[45]), tmp_path)  # same-length flanks
    assert c[2] >= 20, c


def test_thresholds(exe, tmp_path):
    w, _ = world("syn")
    rng = np.random.default_rng(12)
    reads = sf.exact_reads(w.t, rng, n_exons=8) + sf.subst_reads(w.t, rng, n_exons=4)
    for opts in (dict(capi.CI_OPTS, min_aln_score=L + 5), dict(capi.CI_OPTS, min_aln_score=L - 1)):
        check(exe, w, opts, reads, tmp_path)


def test_benchmark_like_batch_every_read_finished_and_none(exe, tmp_path):
    w, _ = world("syn")
    bases, off, _ = synth.simulate_reads(w.t, 3000, L, sub_rate=0.01, indel_rate=0.001, stream=100)
    c = check(exe, w, capi.CI_OPTS, (bases, off), tmp_path)
    assert c[0] >= 300 and c[2] >= 150, c
    out, _ = sf.run_host(exe, w, capi.CI_OPTS, bases, off, tmp_path)
    o = off.astype(np.int64)
    for what, expect in ((1, "all"), (0, "none")):
        reads = [bases[o[i]: o[i + 1]] for i in np.nonzero(out["what"] == what)[0]]
        check(exe, w, capi.CI_OPTS, reads, tmp_path, expect=expect)


def test_micro_exon_reference_and_contig_ends(exe, tmp_path):
    w, _ = world("micro")
    rng = np.random.default_rng(13)
    fwd = sf.forward(w.t)
    reads = sf.exact_reads(w.t, rng) + sf.subst_reads(w.t, rng, n_exons=6)
    reads += [fwd[:L], fwd[-L:], refdata.revcomp(fwd[:L]), refdata.revcomp(fwd[-L:])]
    c = check(exe, w, gc.MICRO_OPTS, reads, tmp_path)
    assert c[0] >= 24 and c[2] >= 20, c


@pytest.mark.parametrize("name", ["planted", "planted64"])
def test_planted_cases(exe, name, tmp_path):
    w, info = world(name)
    rng = np.random.default_rng(14)
    fwd = sf.forward(w.t)
    check(exe, w, capi.CI_OPTS, sf.must_leave_reads(w.t, info, rng), tmp_path)
    a, b, _, _ = info["overlap"]
    reads = [fwd[s: s + L] for s in range(a, b - L + 1, 7)]
    reads += [sf.substitute(r, p, rng) for r in reads for p in (20, 45, L - 21)]
    m0, m1 = info["minus"]
    ends = sf.both_strands([fwd[s: s + L] for s in (m0, m0 + 1, m1 - L, m1 - L - 1, m0 - 1, m1 - L + 1)] * 2)
    reads += ends + [sf.substitute(r, 45, rng) for r in ends]
    for opts in (capi.DEFAULT_OPTS, capi.CI_OPTS):
        c = check(exe, w, opts, reads, tmp_path)
        assert c[0] >= 10 and c[2] >= 10, c


def test_mixed_lengths_and_the_slow_class(exe, tmp_path):
    w, _ = world("syn")
    rng = np.random.default_rng(16)
    fwd = sf.forward(w.t)
    ex = max(sf.exons_forward(w.t), key=lambda e: e[1] - e[0])
    reads = [fwd[ex[0]: ex[0] + n] for n in (30, 60, 91, 120, 150, min(ex[1] - ex[0], 300))]
    reads += [sf.substitute(r, len(r) // 2, rng) for r in reads]
    g0 = int(w.t["refs"][0]["len"]) - 3000
    reads.append(fwd[g0: g0 + 1500])
    c = check(exe, w, capi.CI_OPTS, reads, tmp_path)
    assert c[0] + c[2] >= 8, c


def test_mixed_batch_with_team_and_heavy_reads(exe, tmp_path):
    w, pos = world("heavy")
    hb, ho = synth.reads_from_positions(w.t, pos[:48] + 40, L, sub_rate=0.01, stream=3)
    sb, so, _ = synth.simulate_reads(w.t, 1500, L, sub_rate=0.01, indel_rate=0.001, stream=4)
    bases = np.concatenate([sb[: 700 * L], hb, sb[700 * L:]])
    off = (np.arange(len(bases) // L + 1, dtype=np.uint64) * np.uint64(L)).astype("<u8")
    m = w.oix.all_smems(sf.sanitise(bases), off, capi.CI_OPTS["min_seed_len"])
    hits = np.diff(m.offsets.astype(np.int64))
    assert (hits >= 32).sum() >= 5 and ((hits >= 8) & (hits < 32)).sum() >= 1, np.sort(hits)[-60:]  # team and heavy lists
    c = check(exe, w, capi.CI_OPTS, (bases, off), tmp_path)
    assert c[0] >= 100 and c[2] >= 50, c


def test_pool_overflow_and_replay(exe, tmp_path):
    w, _ = world("syn")
    bases, off, _ = synth.simulate_reads(w.t, 2000, L, sub_rate=0.01, indel_rate=0.001, stream=102)
    for caps in (dict(ops_cap=8192), dict(cand_cap=64), dict(smem_cap=256), dict(ops_cap=64)):
        c = check(exe, w, capi.CI_OPTS, (bases, off), tmp_path, pool_caps=caps)
        assert c[0] >= 200 and c[2] >= 100, c


def test_the_op_run_survives_runs_without_the_finisher(exe, tmp_path):
    """One aligner, the finisher on, then a run that does not use it -- both classes switched off, the problem-parallel path,
    a batch of slow-class reads only, a batch of other reads with the finisher on -- then on again: the run of op bytes at the
    front of the pool, written once, must still be what the finished reads' op streams point into (records, op streams and
    counters of every batch against the oracle; the last one with the host program's finished counts)."""
    w, _ = world("syn")
    opts = capi.CI_OPTS
    fwd = sf.forward(w.t)
    b1, o1, _ = synth.simulate_reads(w.t, 1500, L, sub_rate=0.01, indel_rate=0.001, stream=110)
    b2, o2, _ = synth.simulate_reads(w.t, 1500, L, sub_rate=0.02, indel_rate=0.002, stream=111)
    g0 = int(w.t["refs"][0]["len"]) - 20000
    slow = refdata.pack_reads([fwd[g0 + 2000 * k: g0 + 2000 * k + 1500] for k in range(4)])  # band beyond four cells per lane
    r1 = w.oix.align_batch(b1, o1, opts, n_threads=8)
    r2 = w.oix.align_batch(b2, o2, opts, n_threads=8)
    rs = w.oix.align_batch(slow[0], slow[1], opts, n_threads=8)
    want = sf.finished_counts(sf.run_host(exe, w, opts, b1, o1, tmp_path)[0])
    assert want[0] >= 150 and want[2] >= 75, want

    def run(a, bases, off, r, what):
        a.reset_counters()
        g = a.align_batch(bases, off)
        gc.assert_batch_equal(g, r)
        gc.assert_counters_match(a.counters(), r.counters, what)

    between = {
        "classes_off": lambda a: (a.debug_set_flags(finish_exact=False, finish_subst=False), run(a, b2, o2, r2, "off"),
                                  a.debug_set_flags(finish_exact=True, finish_subst=True)),
        "tpr": lambda a: (a.debug_set_flags(tpr=True), run(a, b2, o2, r2, "tpr"), a.debug_set_flags(tpr=False)),
        "all_slow": lambda a: run(a, slow[0], slow[1], rs, "slow"),
        "other_batch": lambda a: run(a, b2, o2, r2, "other"),
    }
    for name, step in between.items():
        a = w.aligner(opts)
        a.debug_set_flags(tpr=False)
        # every batch of the case once, so that the pools have their final sizes: a pool that grew in the last run would be
        # a new allocation, with a newly written run, and hide what the case is about
        run(a, b2, o2, r2, name + " sizing")
        run(a, slow[0], slow[1], rs, name + " sizing")
        run(a, b1, o1, r1, name + " first")
        assert a.debug_smem_finish_stats() == want, name
        step(a)
        run(a, b1, o1, r1, name + " last")
        assert a.debug_smem_finish_stats() == want, name
        a.close()
