"""CPU side of the device BGZF inflater (include/thermite_io.h: thm_batch_upload_fastq_bgzf): the ABI, and the decode
rules (thermite_amd/csrc/inflate_device.h, the text kernels_inflate.hip spreads over a wavefront) run serially on the
host by tests/cpp/inflate_model_main.cpp over every fixture of tests/inflate_common.py -- against gzip.decompress for
the well-formed ones, against the expected reason for the corrupt ones -- plainly and under AddressSanitizer + UBSan:
the gate before a corrupt byte reaches a device."""
import ctypes
import gzip
import os
import re
import subprocess

import pytest

import fastq_device_common as fc
import inflate_common as ic
from thermite_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["thm_batch_upload_fastq_bgzf"]
DEBUG_SYMBOLS = ["thm_debug_bgzf_inflate", "thm_debug_fastq_bgzf_blocks"]
_WELL, _NOT, _CORRUPT = ic.well_formed(), ic.not_for_device(), ic.corrupt()
HEAD_LENS = (0, 1, 3, 17)   # member outputs on every alignment mod 16 between them (the multi-member fixtures do the rest)


# ------------------------------------------------------------------ the ABI
def test_abi_symbols_and_info_layout(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "thermite_io.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert s in capi.IO_ABI_SYMBOLS
        assert hasattr(capi.lib(), s), "missing export: " + s
    assert set(re.findall(r"\b(thm_[a-z0-9_]+)\s*\(", hdr)) == set(capi.IO_ABI_SYMBOLS)
    for s in DEBUG_SYMBOLS + ["thm_debug_fastq_device_blocks"]:
        assert hasattr(capi.lib(), s) and s not in hdr, s
    core = open(os.path.join(ROOT, "include", "thermite.h")).read()
    assert "THM_N_TIMINGS = 8" in core and capi.N_TIMINGS == 8   # the times live in the info struct
    assert ctypes.sizeof(capi.FastqUploadInfo) == 32
    fields = [f for f, _ in capi.FastqBgzfInfo._fields_]
    assert fields == ["n_reads", "n_bases", "n_name_bytes", "n_lines", "n_members", "n_inflated_bytes", "tail", "tail_len",
                      "inflated_on_device", "parsed_on_device", "inflate_ms", "parse_ms"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "thermite_io.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(thm_fastq_bgzf_info));\n' +
                   "".join('  printf(" %%zu", offsetof(thm_fastq_bgzf_info, %s));\n' % f for f in fields) +
                   '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True).stdout.split()]
    want = [ctypes.sizeof(capi.FastqBgzfInfo)] + [getattr(capi.FastqBgzfInfo, f).offset for f in fields]
    assert got == want and ctypes.sizeof(capi.FastqBgzfInfo) == 80


def test_cpp_header_has_the_upload_call(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#include "thermite.hpp"\nauto p1 = &thermite::Aligner::upload_fastq_bgzf;\nint main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-fsyntax-only", str(src)])


def test_null_arguments_need_no_device():
    L = capi.lib()
    info = capi.FastqBgzfInfo()
    m = ctypes.create_string_buffer(ic.EOF_BLOCK)
    assert L.thm_batch_upload_fastq_bgzf(None, None, 0, m, 28, b"p", 1, 1, ctypes.byref(info)) == capi.ERR_INVALID_ARG
    assert L.thm_batch_upload_fastq_bgzf(None, None, 0, None, 0, b"p", 1, 1, None) == capi.ERR_INVALID_ARG
    n = ctypes.c_uint64(0)
    out = ctypes.create_string_buffer(64)
    assert L.thm_debug_bgzf_inflate(None, m, 28, out, 64, ctypes.byref(n)) == capi.ERR_INVALID_ARG
    c = (ctypes.c_uint64 * 4)()
    assert L.thm_debug_fastq_bgzf_blocks(None, c) == capi.ERR_INVALID_ARG


# ------------------------------------------------------------------ the fixtures themselves
def test_the_fixtures_are_what_they_claim():
    for name, f in _WELL.items():
        assert gzip.decompress(f.members) == f.data, name
        assert len(f.data) <= 65536 * len(ic.split_members(f.members))
    sizes = {len(gzip.decompress(m)) for f in _WELL.values() for m in ic.split_members(f.members)}
    assert {0, 1, 0xff00, 65536} <= sizes
    assert {len(ic.split_members(f.members)) for f in _WELL.values()} >= {1, 2, 40, 65}
    for name, f in _NOT.items():
        assert gzip.decompress(f.members) == f.data, name


@pytest.mark.parametrize("name", list(_NOT) + list(_CORRUPT))
def test_the_host_path_ends_the_odd_ones_as_the_tests_expect(name, tmp_path):
    """the reference of the GPU tests for these: a batch (valid gzip the device does not take) or ERR_IO (corrupt)"""
    if name in _NOT:
        f = _NOT[name]
        if f.fastq:
            outcome, _ = ic.host_outcome_gz(tmp_path, name, f.members)
            want, _ = fc.host_outcome(tmp_path, name, f.data)
            assert outcome[0] == "batch" and fc.batches_differ(outcome[1], want[1]) is None
        else:   # not FASTQ: the host inflater's bytes alone
            p = tmp_path / (name + ".gz")
            p.write_bytes(f.members)
            assert capi.debug_gunzip(p, chunk=1 << 16) == f.data == gzip.decompress(f.members)
    else:
        outcome, path = ic.host_outcome_gz(tmp_path, name, _CORRUPT[name][0])
        assert outcome[0] == "error" and outcome[1] == capi.ERR_IO and "gzip read error in " + path in outcome[2], outcome


# ------------------------------------------------------------------ the model
def _build(tmp, sanitize):
    exe = tmp / ("inflate_model" + ("_asan" if sanitize else ""))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "thermite_amd", "csrc")] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "inflate_model_main.cpp"), "-o", str(exe)])
    return exe


def _run_all(exe, tmp, head_len, env=None):
    """every fixture through one run of the program, the corrupt ones first -> name -> ('ok', n, paths, bytes) |
    ('declined', member, status, paths) | ('walk',)"""
    inputs = [(k, v[0]) for k, v in _CORRUPT.items()] + [(k, v.members) for k, v in _NOT.items()] + \
             [(k, v.members) for k, v in _WELL.items()]
    args = []
    for k, data in inputs:
        (tmp / (k + ".in")).write_bytes(data)
        args += [str(tmp / (k + ".in")), str(tmp / (k + ".%d.out" % head_len))]
    r = subprocess.run([str(exe), str(head_len)] + args, capture_output=True, env=env)
    assert r.returncode == 0, r.stderr.decode()[-4000:]
    res = {}
    for k, _ in inputs:
        out = (tmp / (k + ".%d.out" % head_len)).read_bytes()
        line, _, rest = out.partition(b"\n")
        w = line.split()
        if w[0] == b"ok":
            assert int(w[3]) == len(rest)
            res[k] = ("ok", int(w[1]), int(w[2]), rest)
        elif w[0] == b"declined":
            res[k] = ("declined", int(w[1]), int(w[2]), int(w[3]))
        else:
            assert line == b"walk"
            res[k] = ("walk",)
    return res


@pytest.fixture(scope="module")
def model_results(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("inflate_model")
    exe = _build(tmp, False)
    return {h: _run_all(exe, tmp, h) for h in HEAD_LENS}


@pytest.mark.parametrize("name", list(_WELL))
def test_the_model_inflates_every_well_formed_fixture(model_results, name):
    f = _WELL[name]
    for h in HEAD_LENS:
        r = model_results[h][name]
        assert r[0] == "ok", (h, r[:3])
        assert r[1] == len(ic.split_members(f.members)) and r[3] == f.data, h


def test_every_path_is_reached_by_a_well_formed_fixture(model_results):
    reached = {k: r[2] for k, r in model_results[0].items() if k in _WELL}
    for bit, what in ic.PATH_NAMES.items():
        assert any(p & bit for p in reached.values()), what
    # and the fixtures named for a path still take it
    expect = {"stored_3000": ic.P_STORED, "stored_two_blocks": ic.P_STORED | ic.P_MULTIBLOCK, "stored_block_of_length_0": ic.P_STORED,
              "fixed_3000_fastq": ic.P_FIXED, "empty_member": ic.P_FIXED, "one_byte": ic.P_FIXED, "dynamic_fastq_level_6": ic.P_DYNAMIC,
              "fibonacci_code_length_15": ic.P_DYNAMIC | ic.P_SUBTABLE, "full_flush_mid_member": ic.P_MULTIBLOCK,
              "single_distance_code": ic.P_DYNAMIC,"run_of_5000": ic.P_OVERLAP, "period_3": ic.P_OVERLAP,
              "hand_matches_fixed_65536": ic.P_STORED | ic.P_FIXED | ic.P_FAR | ic.P_OVERLAP | ic.P_MULTIBLOCK,
              "hand_matches_dynamic_65536": ic.P_STORED | ic.P_DYNAMIC | ic.P_FAR | ic.P_OVERLAP | ic.P_MULTIBLOCK}
    for name, bits in expect.items():
        assert reached[name] & bits == bits, (name, reached[name])


@pytest.mark.parametrize("name", list(_NOT))
def test_the_walk_turns_away_what_is_not_bgzf(model_results, name):
    for h in HEAD_LENS:
        assert model_results[h][name] == ("walk",), name


@pytest.mark.parametrize("name", list(_CORRUPT))
def test_the_model_declines_every_corrupt_fixture_for_its_reason(model_results, name):
    _, reasons = _CORRUPT[name]
    for h in HEAD_LENS:
        r = model_results[h][name]
        if reasons is None:
            assert r == ("walk",)
        else:
            assert r[0] == "declined" and r[1] == 0 and r[2] in reasons, r


def test_the_model_is_clean_under_the_sanitizers(tmp_path, model_results):
    """a stand-alone program with the sanitizers linked in (nothing is preloaded): every fixture, corrupt ones first,
    with the buffers cut to the byte; the outcomes are those of the plain build"""
    exe = _build(tmp_path, True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for h in (0, 3):
        got = _run_all(exe, tmp_path, h, env)
        assert got == model_results[h]


def test_host_deflate_blocks_inflate_in_the_model(tmp_path):
    """a block from the host writer's deflate_block, framed: the project's own encoder is among the inputs"""
    text = ic.fastq_text(30000, 15)
    payload = capi.debug_deflate_block(text)
    m = ic.frame(payload, text)
    assert gzip.decompress(m) == text
    exe = _build(tmp_path, False)
    (tmp_path / "own.in").write_bytes(m)
    subprocess.check_call([str(exe), "5", str(tmp_path / "own.in"), str(tmp_path / "own.out")])
    line, _, rest = (tmp_path / "own.out").read_bytes().partition(b"\n")
    assert line.split()[0] == b"ok" and rest == text


def test_an_incomplete_code_is_taken_as_the_host_inflater_takes_it(tmp_path):
    """zlib rejects a literal/length code that leaves code space unused; GzInflater, whose bytes or error are the result
    of the call on every input, decodes it (unassigned entries are an error only when the stream walks into one).  The
    device rules must agree with GzInflater, not with zlib: both give the same bytes here."""
    lit = [0] * 286
    lit[65] = lit[66] = lit[256] = 2          # three codes of two bits: a quarter of the code space is unassigned
    data = b"ABBA" * 5

    def build(b):
        ic.dynamic_header(b, True, lit, [1] + [0] * 29)
        ic.put_tokens(b, list(data), ic.canonical(lit), {})
        b.code(*ic.canonical(lit)[256])
    b = ic.Bits()
    build(b)
    m = ic.frame(b.bytes(), data)
    with pytest.raises(Exception):
        gzip.decompress(m)
    p = tmp_path / "incomplete.gz"
    p.write_bytes(m)
    assert capi.debug_gunzip(p, chunk=1 << 16) == data
    exe = _build(tmp_path, False)
    subprocess.check_call([str(exe), "0", str(p), str(tmp_path / "incomplete.out")])
    line, _, rest = (tmp_path / "incomplete.out").read_bytes().partition(b"\n")
    assert line.split()[0] == b"ok" and rest == data
