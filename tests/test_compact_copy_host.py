"""CPU: the compact stage's op-stream copy and the reach of its GPU test.

  - thermite_amd/csrc/compact_copy.h compiles without the HIP runtime; tests/cpp/compact_copy_main.cpp runs its functions
    with 16 simulated lanes, in the kernel's order, over a memory that checks every access: every source and destination
    residue mod 4 with every length 0..300, 1000 and 4099, against memcpy.  Built as tests/test_extend_plan_host.py
    builds its program, plain and under the host sanitizers, and run directly.
  - the batches of tests/test_gpu_compact_tiles.py (compact_tiles_common.py) mean something only if the oracle's result
    on them has reads on both sides of COMPACT_HEAVY_N, both kinds of alignment, every residue of destination and length,
    and streams beyond one and beyond four trips of a group (256 and 1024 bytes).  That is asserted here, where no
    device is involved."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as orc
from thermite_amd import capi

import compact_tiles_common as cc
from gpu_common import ALN_EXONIC, COMPACT_HEAVY_N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_program(tmp_dir, sanitizers=False):
    exe = os.path.join(str(tmp_dir), "compact_copy_main" + ("_san" if sanitizers else ""))
    extra = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if sanitizers else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + extra +
                          ["-I" + os.path.join(ROOT, "thermite_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "compact_copy_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("sanitizers", [False, True], ids=["plain", "sanitizers"])
def test_copy_against_memcpy(sanitizers, tmp_path):
    r = subprocess.run([host_program(tmp_path, sanitizers)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    m = re.fullmatch(r"cases (\d+) checks (\d+)\n", r.stdout)
    # 4 source residues x 4 destination residues x (lengths 0..300, 1000, 4099): the grid does not shrink unnoticed
    assert m and int(m.group(1)) == 4 * 4 * 303 and int(m.group(2)) > 500 * int(m.group(1)), r.stdout


@pytest.fixture(scope="module")
def results():
    t = cc.tables()
    oix = orc.Index(t, sa=capi.build_suffix_array(t["text"]))
    return {key: (off, cc.oracle(oix, key, bases, off)) for key, bases, off in cc.all_batches()}


def test_heavy_limit_is_the_kernels():
    assert COMPACT_HEAVY_N == 8  # kernels_compact.hip; the families of 8 and 9 copies stand on either side of it


def test_boundary_batches_place_their_reads(results):
    for n in cc.BOUNDARY_NS:
        for swap in (False, True):
            _, _, zero_slots, heavy_slots = cc.boundary_batch(n, swap)
            off, r = results[("boundary", n, swap)]
            n_alns = np.diff(r.offsets.astype(np.int64))
            assert len(n_alns) == n
            assert all(n_alns[s] == 0 for s in zero_slots) and all(n_alns[s] > COMPACT_HEAVY_N for s in heavy_slots)
            slots = set(zero_slots) | set(heavy_slots)
            for b in range(cc.COMPACT_TILE, n + 2, cc.COMPACT_TILE):
                assert (b - 1 >= n or b - 1 in slots) and (b >= n or b in slots)
                if b < n:  # one of each at the boundary, the other way round with swap
                    assert (n_alns[b - 1] == 0) != (n_alns[b] == 0)
                    other = np.diff(results[("boundary", n, not swap)][1].offsets.astype(np.int64))
                    assert (n_alns[b - 1] == 0) != (other[b - 1] == 0)
        # first read without an alignment, last read beyond the limit: in one of the two variants at least, in both
        # where no boundary claims the slot
        firsts = [np.diff(results[("boundary", n, s)][1].offsets.astype(np.int64))[0] for s in (False, True)]
        lasts = [np.diff(results[("boundary", n, s)][1].offsets.astype(np.int64))[-1] for s in (False, True)]
        assert min(firsts) == 0 and max(lasts) > COMPACT_HEAVY_N
        if n > 1:
            assert max(firsts) == 0
        if n % cc.COMPACT_TILE > 1:
            assert min(lasts) > COMPACT_HEAVY_N
    # a tile with more alignments than the kernel holds descriptors for at once (COMPACT_SLOTS = 512)
    off, r = results[("boundary", 2 * cc.COMPACT_TILE + 1, False)]
    assert int(r.offsets[cc.COMPACT_TILE]) > 512


def test_batches_reach_every_case_of_the_copy(results):
    n_alns = np.concatenate([np.diff(r.offsets.astype(np.int64)) for _, r in results.values()])
    for c in (0, 1, 2, COMPACT_HEAVY_N, COMPACT_HEAVY_N + 1):
        assert (n_alns == c).sum() >= 20, c
    alns = np.concatenate([r.alns for _, r in results.values()])
    exonic = alns["aln_type"] == ALN_EXONIC
    assert exonic.sum() >= 50 and (~exonic).sum() >= 50
    assert (alns["tx_ops_len"][exonic] > 0).all() and (alns["tx_ops_len"][~exonic] == 0).all()
    # destinations and lengths of either stream, from the oracle's offsets
    for dst, ln in ((alns["ops_off"], alns["ops_len"]), (alns["tx_ops_off"][exonic], alns["tx_ops_len"][exonic])):
        assert (np.bincount((dst % 4).astype(np.int64), minlength=4) >= 5).all()
        assert (np.bincount((ln % 4).astype(np.int64), minlength=4) >= 5).all()
        assert (ln > 256).sum() >= 1 and (ln > 1024).sum() >= 1
    # ... and the two together, for the genome stream: every head with every tail
    head = (-alns["ops_off"].astype(np.int64)) % 4
    tail = (alns["ops_len"].astype(np.int64) - head) % 4
    assert (np.bincount(head * 4 + tail, minlength=16) >= 1).all()


def test_ragged_batch_has_long_reads_with_both_streams(results):
    off, r = results[("ragged",)]
    lens = np.diff(off.astype(np.int64))
    assert lens.min() == 60 and ((lens >= 60) & (lens <= 120)).sum() >= 3 * cc.COMPACT_TILE - 11
    first = r.offsets.astype(np.int64)[:-1]
    n_alns = np.diff(r.offsets.astype(np.int64))
    for L in (250, 1000):
        idx = np.nonzero((lens == L) & (n_alns > 0))[0]
        assert len(idx) >= 5
        tx = r.alns["tx_ops_len"][first[idx]]
        assert (tx > 0).sum() >= 1 and (tx == 0).sum() >= 1, L
    long_ops = r.alns["ops_len"][first[np.nonzero((lens >= 1000) & (n_alns > 0))[0]]]
    assert (long_ops > 1024).sum() >= 1


def test_empty_batch_has_no_alignment(results):
    off, r = results[("empty",)]
    assert len(off) - 1 == 2 * cc.COMPACT_TILE and int(r.offsets[-1]) == 0
