"""-m gpu: every kernel variant behind a run-time knob against the oracle.

INTEGRATION.md section 6 lists the environment knobs and says that none of them changes a result.  Several select other
device code (THM_SEED_FILL, THM_COMPACT_K, THM_HIT_GL, THM_EXT_MINW*), others another split of the work
(THM_TEAM_DIV_PER_CU, THM_TPR_ROUNDS, THM_SWG_BPC).  Most are read once per process, so each case starts
tests/knob_child.py in a fresh process with the knob in its environment, loads what it saved, asserts from the
thm_debug_knobs report that the knob arrived (a misspelled variable fails here) and compares with the oracle's result:
byte identity, the counter relations of gpu_common.check_align and the SMEM comparison of check_smems.  Each workload
(tests/knob_common.py) is built once and the oracle runs once per workload; every workload states on oracle or
smems_batch output, or on the problem-parallel stats, that it reaches the code it is meant for.

Child processes: one at a time, each under a time limit (a safety stop, far above the measured time).  When a child
ends by a signal or the limit, or reports a memory fault, every later test of this module fails at once with that
child's stderr and starts nothing."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from oracle import pyoracle as orc
from thermite_amd import capi

import knob_common as kc
from gpu_common import COMPACT_HEAVY_N, TEAM_HITS, TEAM_MAX_HITS, World, assert_batch_equal, assert_counters_match, assert_swg_equal

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "knob_child.py")
TEAM_MIN_HITS, TPR_MAX_HITS = 32, 32  # launch.h, extend_plan.h
# seconds; the child's wall time (interpreter start, workload, index, device runs, saving) measured at first run beside it
LIMITS = {
    "fill": 120,      # 2 s
    "compact": 180,   # 2.1 s
    "tpr": 90,        # 1.3 s (the first child of a session; 0.5 s afterwards)
    "minw12": 90,     # 0.6 s
    "minw34": 90,     # 0.7 s
    "team_div": 180,  # 2.1 s
    "swg": 90,        # 1.3 s
}
_dead_child = None  # the latch: what the first child that died left on stderr


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_dead_child():
    if _dead_child is not None:
        pytest.fail("an earlier child process died; nothing more is started.  Its stderr:\n" + _dead_child)


def run_child(tmp_path, workload, wide, env, tpr=None, rounds=0):
    """knob_child.py in a fresh process whose environment is this one's plus `env`; returns the saved arrays"""
    global _dead_child
    out = str(tmp_path / "out.npz")
    cmd = [sys.executable, CHILD, workload, "64" if wide else "32", out]
    if tpr is not None:
        cmd += ["--tpr", str(int(tpr))]
    if rounds:
        cmd += ["--rounds", str(rounds)]
    try:
        p = subprocess.run(cmd, env=dict(os.environ, **env), timeout=LIMITS[workload], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           universal_newlines=True)
    except subprocess.TimeoutExpired as e:
        _dead_child = "%r with %r: no end after %d s\n%s" % (cmd[2:], env, LIMITS[workload], e.stderr or "")
        pytest.fail(_dead_child)
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139) or "an illegal memory access was encountered" in p.stderr:
        _dead_child = "%r with %r: exit status %d\n%s" % (cmd[2:], env, p.returncode, p.stderr[-4000:])
        pytest.fail(_dead_child)
    assert p.returncode == 0, p.stderr[-4000:]
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------ workloads and the oracle's results, once each
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def n_cu():
    return _once("n_cu", kc.device_n_cu)


def workload(name):
    return _once(("w", name), lambda: kc.build(name, n_cu() if name == "compact" else kc.N_CU_DEFAULT))


def world(name, wide=False):
    return _once(("world", name, wide), lambda: World(workload(name)["tables"], wide))


def oracle(name):
    """per run of the workload: (alignments, SMEMs or None, alignments of the second batch or None); for swg: the
    oracle's result per problem set.  Oracle time on 16 threads, measured: compact (98 391 reads) 3 s, fill 2 s, every
    other workload below 1 s."""
    def make():
        w = workload(name)
        if "swg" in w:
            return [orc.swg_extend_batch(xb, xo, yb, yo, bw, xd, max_bw) for xb, xo, yb, yo, bw, xd, max_bw in w["swg"]]
        oix = world(name).oix
        refs = []
        for r in w["runs"]:
            ref = oix.align_batch(r["bases"], r["off"], r["opts"], n_threads=16)
            assert ref.counters[15] == 0, "oracle saw reads where the reference would panic"
            second = oix.align_batch(r["second"][0], r["second"][1], r["opts"], n_threads=16) if r["second"] is not None else None
            n = min(r.get("smem_reads", len(r["off"]) - 1), len(r["off"]) - 1)
            mems = oix.all_smems(r["bases"], r["off"][: n + 1], r["smem_k"]) if r["smem_k"] is not None else None
            refs.append((ref, mems, second))
        return refs
    return _once(("oracle", name), make)


def compare(name, out):
    """what gpu_common.check_align and check_smems assert, on the arrays a run of the workload left"""
    w = workload(name)
    if "swg" in w:
        for i, ref in enumerate(oracle(name)):
            assert_swg_equal(out["swg_alns%d" % i], out["swg_ops%d" % i], ref)
            c = out["swg_counters%d" % i]
            assert c[9] == ref.counters[9] and c[10] <= ref.counters[10] and c[11] <= ref.counters[11]
        return
    for i, (r, (ref, mems, second)) in enumerate(zip(w["runs"], oracle(name))):
        if mems is not None:
            n = len(mems.offsets) - 1  # (all reads, or the front of the batch: smem_reads)
            assert np.array_equal(out["smem_off%d" % i][: n + 1], mems.offsets), "run %d: hit counts differ" % i
            for f in ("ref_idx", "query_idx", "len"):
                bad = np.nonzero(out["smems%d" % i][f][: len(mems.mems)] != mems.mems[f])[0]
                assert len(bad) == 0, "run %d: %s differs at mem %d" % (i, f, bad[0])
        for rep, want in (("a", ref), ("b", second)):
            if want is None:
                continue
            key = "%d%s" % (i, rep)
            g = types.SimpleNamespace(n_reads=len(out["off" + key]) - 1, offsets=out["off" + key], alns=out["alns" + key], ops=out["ops" + key])
            assert int(out["n_failed" + key][0]) == 0 and not out["status" + key].any(), "run " + key
            try:
                assert_batch_equal(g, want)
            except AssertionError as e:
                raise AssertionError("run %s: %s" % (key, e))
            assert_counters_match(out["counters" + key], want.counters, key)


def knobs_of(out):
    return capi.knobs_dict(out["knobs"])


def hits_of(out, i=0):
    return np.diff(out["smem_off%d" % i].astype(np.int64))


# ------------------------------------------------------------------ THM_SEED_FILL
def test_fill_workload_has_the_edges():
    w = workload("fill")
    for i, (r, k) in enumerate(zip(w["runs"][:2], (12, 20))):
        lens = np.diff(r["off"].astype(np.int64))
        npos = lens - k + 1
        assert set(range(8)) <= set((npos[npos > 1] % 8).tolist())       # every residue of PROBE_STRIDE
        assert (lens == k).any() and (lens == k + 1).any() and (lens < k).any() and (lens == 0).any()
        assert (lens > 255).sum() >= 50                                    # the long class
        assert lens[-1] <= k + 2 and lens[-7:].max() <= k + 2             # the batch ends with short reads
        b = r["bases"]
        assert (b == ord("N")).sum() > 100 and ((b >= 97) & (b <= 122)).sum() > 1000
        first, last = b[r["off"][:-1][lens > 2].astype(np.int64)], b[r["off"][1:][lens > 2].astype(np.int64) - 1]
        assert (first == ord("N")).any() and ((last == ord("N")) | (last == ord("a"))).any()
        ref, mems, _ = oracle("fill")[i]
        assert len(ref.alns) > 1500 and len(mems.mems) > 3000
    lens = np.diff(w["runs"][2]["off"].astype(np.int64))
    assert lens.max() == 21 and (lens == 20).any() and len(lens) > 256      # nothing to probe: no cell is listed
    assert len(w["runs"][3]["off"]) == 1                                    # the empty batch
    # the big run: more listed cells than the fixed grid has threads, so seed_fill_kernel from the fixed grid (mode 1) and
    # the key, scatter and bucketed kernels (mode 2) go through their grid-stride loops more than once
    big = w["runs"][4]
    lens = np.diff(big["off"].astype(np.int64))
    cells = (np.maximum(lens - kc.FILL_BIG_K + 1, 1) + kc.PROBE_STRIDE - 1) // kc.PROBE_STRIDE
    assert cells.sum() * kc.PROBE_STRIDE > kc.FILL_FIXED_THREADS
    listed = kc.fill_listed_cells_at_least(w["tables"], big["bases"], big["off"], kc.FILL_BIG_K)
    assert listed * kc.PROBE_STRIDE > kc.FILL_FIXED_THREADS, listed
    ref, mems, _ = oracle("fill")[4]
    assert len(ref.alns) > 1000 and len(mems.mems) > 3000


@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
@pytest.mark.parametrize("mode", [1, 2])
def test_seed_fill_modes(tmp_path, mode, wide):
    """mode 1: seed_fill_kernel from a fixed grid; mode 2: keys, scan, scatter, bucketed probes.  After each batch the same
    aligner aligns the batch in the opposite read order: every buffer of the fill stage (matching statistics, keys,
    permutation) then needs other contents, and the histogram of mode 2 its reset."""
    out = run_child(tmp_path, "fill", wide, {"THM_SEED_FILL": str(mode)})
    assert knobs_of(out)["seed_fill"] == mode
    compare("fill", out)


def test_seed_fill_default_in_this_process():
    out = kc.run_workload(workload("fill"), world("fill").ix)
    assert knobs_of(out)["seed_fill"] == 0
    compare("fill", out)


# ------------------------------------------------------------------ THM_COMPACT_K
def _assert_compact_reach(k_chains):
    w = workload("compact")
    ref = oracle("compact")[0][0]
    n = np.diff(ref.offsets.astype(np.int64))
    ng = w["n_groups"]
    assert ng == n_cu() * 128 and len(n) == 3 * ng + 16 * 5 + 7
    lens = np.diff(w["runs"][0]["off"].astype(np.int64))
    for k in range(1, k_chains):
        x, types_ = n[k * ng:], ref.alns["aln_type"][int(ref.offsets[k * ng]):]
        assert (x == 0).any() and (x == 1).any() and ((x >= 2) & (x <= COMPACT_HEAVY_N)).any() and (x > COMPACT_HEAVY_N).any(), (k, np.bincount(x))
        assert (x == COMPACT_HEAVY_N).any() and (x == COMPACT_HEAVY_N + 1).any()
        assert (types_ == 0).any() and (types_ != 0).any()   # exonic and not
        assert len(set(lens[k * ng:].tolist())) > 20          # ragged: every chain has its own xlen
    # neighbouring chains of one group hold reads of different kinds
    assert ng % kc.COMPACT_KINDS != 0


@pytest.mark.parametrize("k", [1, 4])
def test_compact_k(tmp_path, k):
    """compact_kernel<1> and <4> on a batch of 3 * n_groups + 87 reads: every chain of a 16-lane group holds reads, with
    0, 1, 2..8 and more than 8 alignments and ragged lengths, and the last stride is ragged"""
    _assert_compact_reach(4)
    out = run_child(tmp_path, "compact", False, {"THM_COMPACT_K": str(k)})
    assert knobs_of(out)["compact_k"] == k and knobs_of(out)["n_cu"] == n_cu()
    compare("compact", out)


def test_compact_k_default_in_this_process():
    """compact_kernel<2> with reads in its second chain that differ from the first chain's in kind and length"""
    _assert_compact_reach(2)
    out = kc.run_workload(workload("compact"), world("compact").ix)
    assert knobs_of(out)["compact_k"] == 2
    compare("compact", out)


# ------------------------------------------------------------------ THM_HIT_GL, THM_TPR_ROUNDS
def _assert_tpr_reach(out, rounds=None):
    hits = hits_of(out)
    for h in (1, 2, TPR_MAX_HITS - 1, TPR_MAX_HITS, TPR_MAX_HITS + 1):
        assert (hits == h).sum() >= 8, (h, np.bincount(hits)[:40])
    st = out["tpr_stats0a"]
    assert st[16] > 1000, st       # DP requests were issued: the reads are dirty
    if rounds == 1:
        assert st[0] > 0 and st[8] > 0, st   # reads left to the wave-per-read kernel because the rounds ran out


@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
@pytest.mark.parametrize("lanes", [1, 2, 8])
def test_hit_lanes(tmp_path, lanes, wide):
    """hit_summary_kernel_gl1 / 2 / 8 of the problem-parallel path"""
    out = run_child(tmp_path, "tpr", wide, {"THM_HIT_GL": str(lanes), "THM_TPR": "1"})
    k = knobs_of(out)
    assert k["hit_gl"] == lanes and k["use_tpr"] == 1
    _assert_tpr_reach(out)
    compare("tpr", out)


def test_tpr_rounds_from_the_environment(tmp_path):
    out = run_child(tmp_path, "tpr", False, {"THM_TPR": "1", "THM_TPR_ROUNDS": "1"})
    k = knobs_of(out)
    assert k["use_tpr"] == 1 and k["tpr_rounds"] == 1
    _assert_tpr_reach(out, rounds=1)
    compare("tpr", out)


@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
@pytest.mark.parametrize("rounds", [1, 2, 3, 8])
def test_tpr_rounds(rounds, wide):
    """debug_set_flags(rounds=) is per aligner: in this process"""
    out = kc.run_workload(workload("tpr"), world("tpr", wide).ix, tpr=True, rounds=rounds)
    assert knobs_of(out)["use_tpr"] == 1 and knobs_of(out)["tpr_rounds"] == rounds
    _assert_tpr_reach(out, rounds=rounds)
    compare("tpr", out)


# ------------------------------------------------------------------ THM_EXT_MINW, THM_EXT_MINW_CPL3, THM_EXT_MINW_WIDE
# what extend_waves_per_simd (kernels_extend.hip) gives for a value of THM_EXT_MINW, per cells per lane: the one-cell
# kernel takes 4, 5 and 6 as they are and everything else as 8, the two-cell kernel 4, 5 and 8 and everything else as 6
# (7 has no kernel of its own: the documented fallbacks)
EXT_MINW = {4: {1: 4, 2: 4}, 6: {1: 6, 2: 6}, 7: {1: 8, 2: 6}, 8: {1: 8, 2: 8}}


def _assert_minw_reach(name, cpls):
    assert [kc.cells_per_lane(bw) for _, bw in kc.MINW_SHAPES[name]] == cpls
    for (L, _), refs in zip(kc.MINW_SHAPES[name], oracle(name)):
        a = refs[0].alns
        assert len(a) > 1500 and ((a["score"] < L) & (a["score"] > 0)).sum() > 1000   # dirty reads: the DP ran


@pytest.mark.parametrize("v", [4, 6, 7, 8])
def test_ext_minw(tmp_path, v):
    """extend_kernel<uint32_t, 1, v> (band +-31) and <uint32_t, 2, v> (band +-61)"""
    _assert_minw_reach("minw12", [1, 2])
    out = run_child(tmp_path, "minw12", False, {"THM_EXT_MINW": str(v)})
    k = knobs_of(out)["ext_minw"]
    assert k[(1, False)] == EXT_MINW[v][1] and k[(2, False)] == EXT_MINW[v][2]
    assert k[(1, True)] == 5 and k[(2, True)] == 5   # the 64-bit kernels have their own knob
    compare("minw12", out)


@pytest.mark.parametrize("v", [3, 5, 6])
def test_ext_minw_cpl3(tmp_path, v):
    """extend_kernel<uint32_t, 3, v> (L 120, band +-90) and <uint32_t, 4, v> (L 157, band +-127), global traces"""
    _assert_minw_reach("minw34", [3, 4])
    out = run_child(tmp_path, "minw34", False, {"THM_EXT_MINW_CPL3": str(v)})
    k = knobs_of(out)["ext_minw"]
    assert k[(3, False)] == v and k[(4, False)] == v
    assert k[(3, True)] == 4 and k[(4, True)] == 4   # 64-bit coordinates: four waves whatever the knob says
    compare("minw34", out)


def test_ext_minw_wide(tmp_path):
    """extend_kernel<uint64_t, 1, 4> and <uint64_t, 2, 4>"""
    _assert_minw_reach("minw12", [1, 2])
    out = run_child(tmp_path, "minw12", True, {"THM_EXT_MINW_WIDE": "4"})
    k = knobs_of(out)["ext_minw"]
    assert k[(1, True)] == 4 and k[(2, True)] == 4
    compare("minw12", out)


# ------------------------------------------------------------------ THM_TEAM_DIV_PER_CU
@pytest.mark.parametrize("div", [1, 1000000])
def test_team_divisor(tmp_path, div):
    """plan_kernel's team threshold min(TEAM_HITS, max(TEAM_MIN_HITS, total_hits / (div * n_cu))): with divisor 1 and
    total_hits >= TEAM_HITS * n_cu it is TEAM_HITS, so the reads of TEAM_MIN_HITS..255 hits stay on the wave-per-read
    kernel's heavy list while the team kernel runs beside it; with a huge divisor it is TEAM_MIN_HITS.  No device output
    exposes the lengths of the two lists: which reads go where is restated here from plan_kernel's formula and the hit
    counts of smems_batch; what the device contributes is the knob report and the result."""
    out = run_child(tmp_path, "team_div", False, {"THM_TEAM_DIV_PER_CU": str(div)}, tpr=False)
    k = knobs_of(out)
    assert k["team_div_per_cu"] == div and k["use_tpr"] == 0
    hits = hits_of(out)
    assert hits.sum() >= TEAM_HITS * k["n_cu"], (hits.sum(), k["n_cu"])
    assert min(TEAM_HITS, max(TEAM_MIN_HITS, hits.sum() // (div * k["n_cu"]))) == (TEAM_HITS if div == 1 else TEAM_MIN_HITS)
    assert (hits < TEAM_MIN_HITS).sum() >= 1000 and ((hits >= TEAM_MIN_HITS) & (hits < TEAM_HITS)).sum() >= 50
    assert (hits >= TEAM_HITS).sum() >= 20
    # the team kernel stays: it leaves at once when more than team_limit = 2 * n_cu reads are on its list (pipeline.hip)
    thr = TEAM_HITS if div == 1 else TEAM_MIN_HITS
    on_team_list = int(((hits >= thr) & (hits <= TEAM_MAX_HITS)).sum())
    assert 20 <= on_team_list <= 2 * k["n_cu"], on_team_list
    compare("team_div", out)


# ------------------------------------------------------------------ THM_SWG_BPC
@pytest.mark.parametrize("bpc", [1, 8])
def test_swg_blocks_per_cu(tmp_path, bpc):
    """grid of swg_batch_kernel; for bands beyond +-127 (cpl == 0) also the number of wave-private scratch slices"""
    assert [s[1] for s in kc.SWG_SETS] == [31, 63, 200]
    out = run_child(tmp_path, "swg", False, {"THM_SWG_BPC": str(bpc)})
    k = knobs_of(out)
    assert k["swg_bpc"] == bpc
    # the grids differ from the default's (4 per CU): more workgroups of four problems than the smaller cap
    assert all((n + 3) // 4 > k["n_cu"] * min(bpc, 4) for _, bw_hi, _, n in kc.SWG_SETS if bw_hi <= 127)
    assert bpc > 1 or (kc.SWG_SETS[2][3] + 3) // 4 > k["n_cu"]
    compare("swg", out)
