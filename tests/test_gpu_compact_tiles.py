"""-m gpu: the compact stage (kernels_compact.hip) against the oracle at the seams of its tiling.  A workgroup takes a tile
of COMPACT_TILE = 256 consecutive reads: a thread per read writes one descriptor per alignment, a 16-lane group per
alignment copies the record and the op streams, aligned dwords with single bytes at either end.

  - batches of 1, T - 1, T, T + 1 and 2 T + 1 reads with a read without alignments and one beyond COMPACT_HEAVY_N on either
    side of every tile boundary, both ways round (compact_tiles_common.boundary_batch);
  - a ragged batch of three tiles with reads of 250, 1000 and 1100 bases among reads of 60..120: streams of every
    residue of destination and length, beyond one and beyond four trips of a group, genome and transcript streams;
  - two tiles without any alignment.

tests/test_compact_copy_host.py asserts on the CPU that the batches reach all of that.  The oracle runs once per batch;
one coordinate width runs everything, the other the ragged batch alone (the compact kernels do not depend on the width).
THM_COMPACT_K = 1 and 4 are covered by tests/test_gpu_knobs.py."""
import numpy as np
import pytest

from thermite_amd import capi

import compact_tiles_common as cc
from gpu_common import COMPACT_HEAVY_N, World, assert_batch_equal, check_align

pytestmark = pytest.mark.gpu

COMPACT_TILE = 256  # kernels_compact.hip


def world(wide):
    return cc.once(("world", wide), lambda: World(cc.tables(), wide))


def oracle(key, bases, off):
    return cc.oracle(world(False).oix, key, bases, off)


def test_tile_size_is_the_kernels():
    assert cc.COMPACT_TILE == COMPACT_TILE and COMPACT_HEAVY_N == 8


@pytest.mark.parametrize("swap", [False, True], ids=["zero_heavy", "heavy_zero"])
@pytest.mark.parametrize("n", cc.BOUNDARY_NS)
def test_tile_boundaries(n, swap):
    bases, off, zero_slots, heavy_slots = cc.boundary_batch(n, swap)
    ref = oracle(("boundary", n, swap), bases, off)
    n_alns = np.diff(ref.offsets.astype(np.int64))
    assert all(n_alns[s] == 0 for s in zero_slots) and all(n_alns[s] > COMPACT_HEAVY_N for s in heavy_slots)
    assert len(zero_slots) + len(heavy_slots) >= 1
    check_align(world(False), bases, off, capi.CI_OPTS, ref=ref)


@pytest.mark.parametrize("wide", [False, True], ids=["c32", "c64"])
def test_ragged_and_long_streams(wide):
    bases, off = cc.ragged_batch()
    ref = oracle(("ragged",), bases, off)
    assert int(ref.alns["ops_len"].max()) > 1024 and int(ref.alns["tx_ops_len"].max()) > 1024
    check_align(world(wide), bases, off, capi.CI_OPTS, ref=ref)


def test_tiles_without_alignments():
    bases, off = cc.empty_batch()
    ref = oracle(("empty",), bases, off)
    assert int(ref.offsets[-1]) == 0
    check_align(world(False), bases, off, capi.CI_OPTS, ref=ref)


def test_one_aligner_across_batches():
    """the batches one after another on one aligner: the heavy list and its counts start again with every run"""
    a = world(False).aligner(capi.CI_OPTS)
    for key, bases, off in (cc.all_batches()[5], cc.all_batches()[-1], cc.all_batches()[-2], cc.all_batches()[1], cc.all_batches()[9]):
        g = a.align_batch(bases, off)
        assert g.n_failed == 0
        assert_batch_equal(g, oracle(key, bases, off))
    a.close()
