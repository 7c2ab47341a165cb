"""CPU side of the text positions kept in single-suffix k-mer table entries (thermite_amd/csrc/lut_direct.h): the decision,
the encode / decode round trips and the plain entries, run on the host by tests/cpp/lut_direct_main.cpp; the exports and
their Python bindings; and that the host's own table stays plain."""
import os
import subprocess

import numpy as np

from thermite_amd import capi, refdata, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_tagging_functions_on_the_host(tmp_path):
    exe = tmp_path / "lut_direct_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "thermite_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "lut_direct_main.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert out[0] == "ok" and int(out[1]) > 100


def test_exports_and_null_arguments_need_no_device():
    L = capi.lib()
    for s in ("thm_debug_seed_direct_stats", "thm_debug_fetch_lut", "thm_debug_host_lut"):
        assert hasattr(L, s), s
    out = np.zeros(4, "<u8")
    assert L.thm_debug_seed_direct_stats(None, capi._ptr(out)) == capi.ERR_INVALID_ARG
    assert L.thm_debug_fetch_lut(None, capi._ptr(out), 32) == capi.ERR_INVALID_ARG
    assert L.thm_debug_host_lut(None, None, None, 0) == capi.ERR_INVALID_ARG


def test_the_host_table_is_plain_at_both_widths():
    """(lo, hi) of every entry are ranks, whatever the device copy will hold: hi - lo counts the kt-mer's occurrences"""
    data = os.path.join(ROOT, "tests", "golden", "data")
    t = refdata.load_reference(os.path.join(data, "test_ref.fasta"), os.path.join(data, "test_ref.gtf"))
    n = len(t["text"])
    tables = {}
    for wide in (False, True):
        ix = capi.Index(t, wide=wide)
        lut = ix.debug_host_lut()
        assert lut.dtype == ("<u8" if wide else "<u4") and lut.shape[0] == 4 ** round(np.log(lut.shape[0]) / np.log(4))
        assert (lut[:, 0] <= lut[:, 1]).all() and int(lut[:, 1].max()) <= n
        assert ix.check_lut()
        tables[wide] = lut.astype(np.uint64)
        ix.close()
    assert np.array_equal(tables[False], tables[True])
    assert ((tables[False][:, 1] - tables[False][:, 0]) == 1).any()
