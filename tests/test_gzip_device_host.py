"""CPU side of the device inflater for plain gzip (include/thermite_io.h: thm_batch_upload_fastq_gzip): the ABI, the host
inflater's resume entry, and the rules (thermite_amd/csrc/gzip_device.h, the text kernels_gzip.hip spreads over
wavefronts) run serially on the host by tests/cpp/gzip_model_main.cpp over every fixture of tests/gzip_common.py, at
every chunk size and in slices with the state carried -- against gzip.decompress for the bytes, against the host path
call by call for consumption and states, against the expected status for what is declined or corrupt -- plainly and under
AddressSanitizer + UBSan: the gate before a corrupt byte reaches a device."""
import ctypes
import gzip
import os
import re
import subprocess
import zlib

import pytest

import gzip_common as gc
from thermite_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WELL, _DECLINED, _CORRUPT = gc.well_formed(), gc.declined(), gc.corrupt()
# the corrupt ones first
_INPUTS = [(k, v[0]) for k, v in _CORRUPT.items()] + [(k, v[0].stream) for k, v in _DECLINED.items()] + [(k, v.stream) for k, v in _WELL.items()]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gzip_model")
    return gc.build_model(tmp), tmp


# ------------------------------------------------------------------ the ABI
def test_abi_symbols_and_layouts(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "thermite_io.h")).read()
    assert re.search(r"\bthm_batch_upload_fastq_gzip\s*\(", hdr) and "thm_batch_upload_fastq_gzip" in capi.IO_ABI_SYMBOLS
    assert hasattr(capi.lib(), "thm_batch_upload_fastq_gzip")
    assert set(re.findall(r"\b(thm_[a-z0-9_]+)\s*\(", hdr)) == set(capi.IO_ABI_SYMBOLS)
    for s in ("thm_debug_gzip_inflate", "thm_debug_fastq_gzip_blocks", "thm_debug_gzip_host_slice"):
        assert hasattr(capi.lib(), s) and s not in hdr, s
    core = open(os.path.join(ROOT, "include", "thermite.h")).read()
    assert "THM_N_TIMINGS = 8" in core and capi.N_TIMINGS == 8
    info = [f for f, _ in capi.FastqGzipInfo._fields_]
    assert info[:11] == ["n_reads", "n_bases", "n_name_bytes", "n_lines", "n_inflated_bytes", "tail", "tail_len", "inflated_on_device",
                         "parsed_on_device", "inflate_ms", "parse_ms"]
    assert info[11:15] == ["n_consumed_bytes", "n_chunks", "n_starts", "decline_reason"]
    state = [f for f, _ in capi.GzipState._fields_]
    assert state == ["window", "window_len", "bit_offset", "in_member", "crc", "member_len", "n_members_done", "stream_offset"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "thermite_io.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(thm_fastq_gzip_info));\n' +
                   "".join('  printf(" %%zu", offsetof(thm_fastq_gzip_info, %s));\n' % f for f in info) +
                   '  printf(" %zu", sizeof(thm_gzip_state));\n' +
                   "".join('  printf(" %%zu", offsetof(thm_gzip_state, %s));\n' % f for f in state) +
                   '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True).stdout.split()]
    want = [ctypes.sizeof(capi.FastqGzipInfo)] + [getattr(capi.FastqGzipInfo, f).offset for f in info] + \
           [ctypes.sizeof(capi.GzipState)] + [getattr(capi.GzipState, f).offset for f in state]
    assert got == want
    assert ctypes.sizeof(capi.GzipState) == 32768 + 16 + 24 and ctypes.sizeof(capi.FastqGzipInfo) == 104


def test_null_arguments_need_no_device():
    L = capi.lib()
    info, st = capi.FastqGzipInfo(), capi.GzipState()
    m = ctypes.create_string_buffer(_WELL["small"].stream)
    assert L.thm_batch_upload_fastq_gzip(None, ctypes.byref(st), None, 0, m, 100, b"p", 1, 1, ctypes.byref(info)) == capi.ERR_INVALID_ARG
    assert L.thm_batch_upload_fastq_gzip(None, None, None, 0, None, 0, b"p", 1, 1, None) == capi.ERR_INVALID_ARG
    n, used = ctypes.c_uint64(0), ctypes.c_uint64(0)
    out = ctypes.create_string_buffer(64)
    assert L.thm_debug_gzip_inflate(None, ctypes.byref(st), m, 100, 0, 1, out, 64, ctypes.byref(n), ctypes.byref(used), None) == capi.ERR_INVALID_ARG
    c = (ctypes.c_uint64 * 4)()
    assert L.thm_debug_fastq_gzip_blocks(None, c) == capi.ERR_INVALID_ARG
    assert L.thm_debug_gzip_host_slice(None, m, 100, 1, out, 64, ctypes.byref(n), ctypes.byref(used)) == capi.ERR_INVALID_ARG
    bad = capi.GzipState()
    bad.bit_offset = 3   # bits consumed of a member header
    assert L.thm_debug_gzip_host_slice(ctypes.byref(bad), m, 100, 1, out, 64, ctypes.byref(n), ctypes.byref(used)) == capi.ERR_INVALID_ARG


# ------------------------------------------------------------------ the fixtures themselves
def test_the_fixtures_are_what_they_claim():
    assert 400000 < len(gc.text()) < 500000 and 2500 < len(gc.small()) < 3500
    for name, f in _WELL.items():
        if name == "bad_magic_second_member":
            d = zlib.decompressobj(31)
            assert d.decompress(f.stream) == f.data and d.eof and d.unused_data[:2] == b"\x1f\x8c"
        else:
            assert gzip.decompress(f.stream) == f.data, name
    assert all(gzip.decompress(f.stream) == f.data for f, _ in _DECLINED.values())
    for name, (stream, _) in _CORRUPT.items():
        if name == "flip_2":    # a reserved flag bit: zlib and GzInflater refuse it, Python's gzip module does not look
            with pytest.raises(zlib.error, match="unknown header flags"):
                zlib.decompressobj(31).decompress(stream)
            continue
        with pytest.raises((OSError, EOFError, zlib.error)):
            gzip.decompress(stream)
    assert len(set(gc.FLIP_BITS)) == 10


def test_the_host_path_takes_every_fixture_whole_and_in_slices():
    """the reference of the model and GPU tests for consumption and errors is sound itself: the bytes, or ERR_IO"""
    for slice_bytes in gc.MODEL_SLICES:
        for name, f in list(_WELL.items()) + [(k, v[0]) for k, v in _DECLINED.items()]:
            calls, data = gc.host_chain(f.stream, slice_bytes)
            assert data == f.data and not isinstance(calls[-1], Exception), (name, slice_bytes)
            assert sum(c[3] for c in calls) == len(f.stream) and calls[-1][4][3] == 0   # all consumed, at a member boundary
        for name, (stream, _) in _CORRUPT.items():
            calls, _ = gc.host_chain(stream, slice_bytes)
            assert isinstance(calls[-1], capi.ThermiteError) and calls[-1].code == capi.ERR_IO, (name, slice_bytes)
            assert "gzip read error in " in str(calls[-1])


# ------------------------------------------------------------------ the model
def _check(results, chunk, slice_bytes):
    """one run of the model over all fixtures against what is expected of each; the flags the well-formed ones walked"""
    flags = 0
    for name, f in _WELL.items():
        m = results[name]
        assert [c.status for c in m.calls] == [0] * len(m.calls), "%s declines at chunk size %d, slices of %d: %r" % (
            name, chunk, slice_bytes, [c for c in m.calls if c.status])
        assert m.data == f.data, (name, chunk, slice_bytes)
        # call by call what the host path consumes and leaves, the window included
        host, _ = gc.host_chain(f.stream, slice_bytes)
        assert [(c.n, c.last_block, c.n_out, c.n_consumed) for c in m.calls] == [h[:4] for h in host], (name, chunk, slice_bytes)
        assert [s.key() for s in m.states] == [h[4] for h in host], (name, chunk, slice_bytes)
        for c in m.calls:
            assert c.n_consumed <= c.n and c.n_refused == 0
            flags |= c.flags
    for name, (f, why) in _DECLINED.items():
        m = results[name]
        assert m.calls[-1].status in why + (gc.TRUNCATED,), (name, chunk, slice_bytes, m.calls[-1])
        assert slice_bytes or m.calls[-1].status in why
    for name, (stream, why) in _CORRUPT.items():
        m = results[name]
        assert m.calls[-1].status != gc.OK, (name, chunk, slice_bytes)
        if why and not slice_bytes:
            assert m.calls[-1].status in why, (name, chunk, m.calls[-1])
        host, _ = gc.host_chain(stream, slice_bytes)
        assert len(m.calls) <= len(host), "the device trusts a call the host inflater fails: %s" % name
    return flags


@pytest.mark.parametrize("chunk", gc.MODEL_CHUNKS)
def test_model_over_every_fixture(model, chunk):
    """bytes, consumption and states at this chunk size, whole and in slices of 7 000 and 20 000 bytes; every path flag
    is reached by well-formed input at the small chunk sizes; no well-formed fixture declines (the cap)"""
    exe, tmp = model
    flags = 0
    for slice_bytes in gc.MODEL_SLICES:
        flags |= _check(gc.run_model(exe, tmp, chunk, slice_bytes, _INPUTS), chunk, slice_bytes)
    if chunk <= 4096:
        missing = [n for b, n in gc.FLAG_NAMES.items() if not flags & b]
        assert not missing, "paths no well-formed fixture walks at chunk size %d: %s" % (chunk, missing)


def test_model_finds_the_many_starts_of_small_blocks(model):
    exe, tmp = model
    r = gc.run_model(exe, tmp, 256, 0, [("mem_level1", _WELL["mem_level1"].stream), ("level0_stored", _WELL["level0_stored"].stream)])
    assert r["mem_level1"].calls[0].n_starts >= 100
    assert r["level0_stored"].calls[0].n_starts == 1    # stored blocks only: no start but the first, one run


def test_model_without_last_block_keeps_the_state_of_a_cut_stream(model):
    """a stream cut mid-block is no error while more may follow: the blocks that ended are out, the rest waits"""
    exe, tmp = model
    stream, data = _WELL["level6"].stream[:100001], gc.text()
    m = gc.run_model(exe, tmp, 4096, 0, [("cut", stream)], last=0)["cut"]
    assert m.calls[-1].status == gc.OK and m.calls[-1].flags & gc.G_ROLLBACK
    assert 0 < m.calls[-1].n_consumed < len(stream) and m.data == data[: len(m.data)] and m.states[-1].in_member == 1
    host, got = gc.host_chain(stream, 0, last=False)
    assert got == m.data and host[-1][4] == m.states[-1].key()


def test_model_under_the_sanitizers(model):
    """stand-alone, buffers cut to the byte, corrupt fixtures first: a read or write out of bounds ends the run"""
    _, tmp = model
    exe = gc.build_model(tmp, sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    for chunk, slice_bytes in ((64, 7000), (4096, 0), (gc.DEFAULT_CHUNK, 20000)):
        _check(gc.run_model(exe, tmp, chunk, slice_bytes, _INPUTS, env=env), chunk, slice_bytes)


# ------------------------------------------------------------------ the host inflater's resume entry
@pytest.mark.parametrize("name", ["level6", "mem_level1"])
def test_resume_entry_from_every_boundary_the_model_reports(model, name):
    """from every state the model leaves between slices -- a block boundary: bit offset, window, CRC, length -- the host
    inflater gives the remaining bytes, and the same verdicts on a trailer with a wrong CRC or ISIZE"""
    exe, tmp = model
    f = _WELL[name]
    m = gc.run_model(exe, tmp, 4096, 3000, [(name, f.stream)])[name]
    assert all(c.status == 0 for c in m.calls)
    # (level 6 cuts this text into seven blocks, memLevel 1 into hundreds)
    assert len({(s.stream_offset, s.bit_offset) for s in m.states}) >= (6 if name == "level6" else 40)
    assert len({s.bit_offset for s in m.states}) >= 4
    done = 0
    bad_crc = f.stream[:-8] + bytes([f.stream[-8] ^ 1]) + f.stream[-7:]
    bad_len = f.stream[:-1] + bytes([f.stream[-1] ^ 1])
    for c, s in zip(m.calls, m.states):
        done += c.n_out
        at = s.stream_offset
        if at == len(f.stream):
            assert s.in_member == 0 and done == len(f.data)
            continue
        st = s.copy()
        got, used = capi.debug_gzip_host_slice(st, f.stream[at:], last_block=True)
        assert got == f.data[done:] and used == len(f.stream) - at and st.in_member == 0 and st.n_members_done == 1
        for bad, what in ((bad_crc, "incorrect data check"), (bad_len, "incorrect length check")):
            st = s.copy()
            with pytest.raises(capi.ThermiteError, match=what):
                capi.debug_gzip_host_slice(st, bad[at:], last_block=True)
            assert st.key() == s.key()      # on an error the state is unchanged
