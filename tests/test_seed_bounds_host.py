"""CPU side of the seed stage's cell rule (thermite_amd/csrc/seed_bounds.h): tests/cpp/seed_bounds_main.cpp derives the
row of match ends through grid bounds, the header's rule and probes and compares it with the row straight from
brute-force matching statistics, over named cases and a seeded random sweep -- built plain and under AddressSanitizer +
UBSan, as a program with its own main; the batch-file road the GPU test uses; and the switch in the bindings."""
import inspect
import subprocess

import numpy as np
import pytest

from thermite_amd import capi

import seed_bounds_common as sb


@pytest.mark.parametrize("sanitizers", [False, True], ids=["plain", "asan_ubsan"])
def test_the_rule_against_brute_force_on_the_host(tmp_path, sanitizers):
    exe = sb.build_host_program(tmp_path, sanitizers)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    lines = out.strip().split("\n")
    assert lines[-1].split()[0] == "ok" and int(lines[-1].split()[1]) > 100000, out
    counts = {}
    for ln in lines[:-1]:
        f = ln.replace(",", "").split()
        counts[f[0]] = (int(f[f.index("off") + 1]), int(f[f.index("on") + 1]))
    for name in ("one_sub_L91", "one_sub_L29", "one_sub_L35", "k40", "two_subs", "duplicate", "empty_bucket", "n_and_contig_end",
                 "indels", "k_is_kt", "k_below_kt", "one_long_among_short", "random_sweep"):
        assert counts[name][1] < counts[name][0], (name, counts[name])
    for name in ("length_k", "length_k_plus_1"):   # no cells: nothing to decide
        assert counts[name][1] == counts[name][0], (name, counts[name])


def test_a_batch_file_gives_the_counts_of_a_model_in_python(tmp_path):
    """one error-free read that is not in the text as a whole (two halves from different places) and one that is: the
    probes of the second are position 0 alone; of the first, position 0, the grid, and the cell around the joint"""
    rng = np.random.Generator(np.random.PCG64(7))
    text = np.concatenate([sb.ACGT[rng.integers(0, 4, 4000)], [ord("$")]]).astype(np.uint8)
    whole = text[100:191]
    joined = np.concatenate([text[1000:1045], text[3000:3046]])
    bases = np.concatenate([whole, joined])
    off = np.array([0, 91, 182], "<u8")
    exe = sb.build_host_program(tmp_path)
    path = str(tmp_path / "two.batch")
    sb.write_batch(path, text, bases, off, 20, 8)
    out = subprocess.run([exe, "--file", path], check=True, capture_output=True, text=True).stdout.split()
    p_off, p_on = int(out[1]), int(out[2])
    # joined: npos = 72, grid 8 .. 64 and 71 (9 probes) + position 0; matches end at 45 for i < 45 and at 91 behind
    # (chance matches across the joint aside).  Rule off: the cells [24, 32] .. [40, 48] hold the zone 25 < i < 45 where
    # MS < k or the end jumps: whole cells, 7 probes each.
    assert p_off >= 1 + 10 + 3 * 7 and p_on < p_off and p_on >= 1 + 10 + 1
    assert subprocess.run([exe, "--file", str(tmp_path / "missing")], capture_output=True).returncode == 2


def test_the_switch_is_in_the_bindings():
    assert "seed_bounds" in inspect.signature(capi.Aligner.debug_set_flags).parameters
    assert capi.lib().thm_debug_set_flags(None, 0x10000) == capi.ERR_INVALID_ARG
