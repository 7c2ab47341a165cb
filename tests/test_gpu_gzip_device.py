"""-m gpu: plain gzip inflated on the device (kernels_gzip.hip, thm_batch_upload_fastq_gzip and its debug hooks, the file
driver's THM_FASTQ_DEVICE=3).  The reference for bytes, consumption and states is the host model of the same rules
(tests/cpp/gzip_model_main.cpp, itself checked against gzip.decompress and the host path in test_gzip_device_host.py);
for batches and errors it is the host path -- GzInflater's resume entry, then fastq_parse_block.  Everything is byte
equality.  No input here is new to the rules: every fixture, the corrupt ones first, has gone through the model under the
sanitizers on the CPU, and the device's answer to a corrupt one is a status word."""
import gzip

import numpy as np
import pytest

import bam_common as bc
import fastq_device_common as fc
import gzip_common as gc
from gpu_common import World
from test_gpu_inflate_device import _concat, _run_both_fetches, _same_results
from thermite_amd import capi

pytestmark = pytest.mark.gpu

_worlds, _sets = {}, {}
_WELL, _DECLINED, _CORRUPT = gc.well_formed(), gc.declined(), gc.corrupt()
_FASTQ = [k for k, f in _WELL.items() if f.fastq]
_INPUTS = [(k, v.stream) for k, v in _WELL.items()]


def _world(key):
    if key not in _worlds:
        _worlds[key] = World(bc.tables(key))
    return _worlds[key]


def _set(name):
    w = _world(bc.REF_OF[name])
    if name not in _sets:
        _sets[name] = bc.read_set(name, w.t)
    return w, _sets[name]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("gzip_model")
    return gc.build_model(tmp), tmp


def _message(e):
    """a gzip error's message behind the path"""
    return str(e).split(": ", 2)[-1]


# ------------------------------------------------------------------ 1. the inflate alone: no host inflater behind it
@pytest.mark.parametrize("chunk", gc.GPU_CHUNKS)
def test_every_well_formed_fixture_inflates_as_the_model_does(model, chunk):
    """bytes, n_consumed, outgoing state, starts and path flags of every well-formed fixture at this chunk size"""
    exe, tmp = model
    want = gc.run_model(exe, tmp, chunk, 0, _INPUTS)
    a = _world("test_ref").a
    for name, f in _WELL.items():
        st = capi.GzipState()
        got, used, counts = a.debug_gzip_inflate(st, f.stream, chunk_bytes=chunk, cap=len(f.data))
        m = want[name]
        assert got == f.data == m.data, (name, chunk)
        assert (used, st.key()) == (m.calls[0].n_consumed, m.states[0].key()), (name, chunk)
        assert counts == (m.calls[0].n_chunks, m.calls[0].n_starts, 0, m.calls[0].flags), (name, chunk, counts, m.calls[0])
        print(name, chunk, "chunks / starts / flags", counts)


@pytest.mark.parametrize("name", ["level6", "mem_level1", "three_members", "flushes"])
def test_slices_with_the_state_carried_inflate_as_the_model_does(model, name):
    exe, tmp = model
    f = _WELL[name]
    m = gc.run_model(exe, tmp, 4096, 7000, [(name, f.stream)])[name]
    a = _world("test_ref").a
    st, at, data = capi.GzipState(), 0, b""
    for k, c in enumerate(m.calls):
        got, used, counts = a.debug_gzip_inflate(st, f.stream[at: at + c.n], chunk_bytes=4096, last_block=c.last_block, cap=1 << 20)
        assert (len(got), used, st.key()) == (c.n_out, c.n_consumed, m.states[k].key()), (name, k)
        assert counts[1:] == (c.n_starts, 0, c.flags)
        data += got
        at += used
    assert data == f.data and at == len(f.stream)
    assert any(c.flags & gc.G_ROLLBACK for c in m.calls)
    if name in ("level6", "three_members"):     # blocks of about 29 KB: calls in which none ends
        assert any(c.n_consumed == 0 for c in m.calls)


@pytest.mark.parametrize("name", list(_DECLINED) + list(_CORRUPT))
def test_the_hook_has_no_fallback(name):
    """what the device does not take is an error of the hook that names the status word, never bytes; the state stays"""
    a = _world("test_ref").a
    stream, why = (_DECLINED[name][0].stream, _DECLINED[name][1]) if name in _DECLINED else _CORRUPT[name]
    st = capi.GzipState()
    with pytest.raises(capi.ThermiteError) as e:
        a.debug_gzip_inflate(st, stream, cap=4 << 20)
    assert e.value.code == capi.ERR_UNSUPPORTED and "declined with status" in str(e.value)
    assert st.key() == capi.GzipState().key()
    if why:
        assert any("declined with status %d at" % s in str(e.value) for s in why), str(e.value)


# ------------------------------------------------------------------ 2. the call: inflate + parse, batch, tail, state
def _chain(a, stream, path, first, then, head=b"", state=None, aligners=None):
    """the stream through the call in slices of `first`, then `then` bytes (0: all that is left), a slice doubled when
    nothing of it was consumed -> (infos, batches, the text consumed by the batches); `aligners`: the calls go to
    these in turn, state and tail handed from one to the next"""
    st = state or capi.GzipState()
    at, size, line, infos, batches = 0, first or len(stream), 1, [], []
    while True:
        n = min(size, len(stream) - at)
        last = at + n == len(stream)
        al = aligners[len(infos) % len(aligners)] if aligners else a
        before = st.key()
        info = al.upload_fastq_gzip(st, stream[at: at + n], head=head, path=path, first_line=line, last_block=last)
        infos.append(info)
        batches.append(al.fetch_reads())
        assert len(batches[-1]["offsets"]) - 1 == info["n_reads"] and info["n_consumed_bytes"] <= n
        if info["n_consumed_bytes"] == 0 and not last:   # no block ended: nothing moved
            assert (info["n_reads"], info["tail"], info["n_inflated_bytes"]) == (0, head, 0) and st.key() == before
        head, line, at = info["tail"], line + info["n_lines"], at + info["n_consumed_bytes"]
        if last:
            return infos, batches, st
        size = size * 2 if info["n_consumed_bytes"] == 0 else (then or len(stream))


@pytest.mark.parametrize("name", _FASTQ)
def test_fastq_fixtures_in_one_call_and_in_slices(name, tmp_path):
    f = _WELL[name]
    a = _world("test_ref").a
    outcome, path = fc.host_outcome(tmp_path, name, f.data)
    assert outcome[0] == "batch"
    want = outcome[1]
    # one call
    c0 = a.debug_fastq_gzip_blocks()
    st = capi.GzipState()
    info = a.upload_fastq_gzip(st, f.stream, path=path)
    print(name, len(f.stream), "->", len(f.data), {k: v for k, v in info.items() if k != "tail"})
    assert info["inflated_on_device"] == 1 and info["parsed_on_device"] == 1 and info["decline_reason"] == 0
    assert info["inflate_ms"] > 0 and info["parse_ms"] > 0 and info["tail"] == b""
    assert (info["n_consumed_bytes"], info["n_inflated_bytes"], info["n_lines"]) == (len(f.stream), len(f.data), 4 * info["n_reads"])
    assert info["n_chunks"] == -(-len(f.stream) // gc.DEFAULT_CHUNK) and 1 <= info["n_starts"] <= info["n_chunks"]
    assert a.debug_fastq_gzip_blocks() == (c0[0] + 1, c0[1], c0[2] + 1, c0[3])
    assert fc.batches_differ(a.fetch_reads(), want) is None
    assert (st.in_member, st.window_len, st.bit_offset, st.stream_offset) == (0, 0, 0, len(f.stream)) and st.n_members_done >= 1
    # slices: a first one in which (for the long members) no block ends, then 60 000 bytes each
    c0 = a.debug_fastq_gzip_blocks()
    infos, batches, st = _chain(a, f.stream, path, 3000, 60000)
    assert fc.batches_differ(_concat(batches), want) is None
    assert sum(i["n_inflated_bytes"] for i in infos) == len(f.data) and st.stream_offset == len(f.stream) and st.in_member == 0
    assert all(i["inflated_on_device"] == 1 and i["decline_reason"] == 0 for i in infos)
    c1 = a.debug_fastq_gzip_blocks()
    assert c1[0] - c0[0] == len(infos) and c1[1] == c0[1] and c1[2] - c0[2] == sum(i["parsed_on_device"] for i in infos)
    if len(f.stream) > 100000:
        assert infos[0]["n_consumed_bytes"] == 0 or name in ("mem_level1", "level0_stored")


@pytest.mark.parametrize("head_len", [1, 3, 17])
def test_a_head_shifts_the_inflated_bytes(head_len, tmp_path):
    text = gc.text(42)
    a = _world("test_ref").a
    outcome, path = fc.host_outcome(tmp_path, "shift", text)
    st = capi.GzipState()
    info = a.upload_fastq_gzip(st, gc.member(text[head_len:]), head=text[:head_len], path=path)
    assert info["inflated_on_device"] == 1 and info["parsed_on_device"] == 1 and info["n_inflated_bytes"] == len(text) - head_len
    assert fc.batches_differ(a.fetch_reads(), outcome[1]) is None


def test_a_call_in_which_no_block_ends_and_an_empty_one():
    a = _world("test_ref").a
    stream = _WELL["level6"].stream
    st = capi.GzipState()
    info = a.upload_fastq_gzip(st, stream[:5000], head=b"@r1 x\nAC", last_block=False)
    assert (info["n_consumed_bytes"], info["n_reads"], info["n_lines"], info["tail"], info["n_inflated_bytes"]) == (0, 0, 0, b"@r1 x\nAC", 0)
    assert info["inflated_on_device"] == 1 and info["parsed_on_device"] == 0 and st.key() == capi.GzipState().key()
    assert len(a.fetch_reads()["offsets"]) == 1
    info = a.upload_fastq_gzip(st, b"", last_block=True)
    assert (info["n_reads"], info["tail"], info["inflated_on_device"], info["n_chunks"]) == (0, b"", 0, 0)
    bad = capi.GzipState()
    bad.in_member, bad.window_len, bad.member_len = 1, 5, 70000     # a window shorter than the member's bytes allow
    with pytest.raises(capi.ThermiteError) as e:
        a.upload_fastq_gzip(bad, stream[:5000])
    assert e.value.code == capi.ERR_INVALID_ARG


# ------------------------------------------------------------------ 3. what the device does not take ends as the host ends it
def _host_calls(stream, first, then):
    """gc.host_chain in the slices of _chain"""
    st, at, size, calls = capi.GzipState(), 0, first or len(stream), []
    while True:
        n = min(size, len(stream) - at)
        last = at + n == len(stream)
        try:
            got, used = capi.debug_gzip_host_slice(st, stream[at: at + n], last_block=last)
        except capi.ThermiteError as e:
            return calls + [e]
        calls.append((len(got), used))
        at += used
        if last:
            return calls
        size = size * 2 if used == 0 else (then or len(stream))


@pytest.mark.parametrize("name", list(_DECLINED))
def test_valid_gzip_the_device_declines_is_inflated_on_the_host(name, tmp_path):
    f, why = _DECLINED[name]
    a = _world("test_ref").a
    c0 = a.debug_fastq_gzip_blocks()
    st = capi.GzipState()
    if f.fastq:
        outcome, path = fc.host_outcome(tmp_path, name, f.data)
        info = a.upload_fastq_gzip(st, f.stream, path=path)
        assert info["inflated_on_device"] == 0 and info["inflate_ms"] == 0 and info["decline_reason"] in why
        assert info["n_inflated_bytes"] == len(f.data) and info["n_consumed_bytes"] == len(f.stream) and info["parsed_on_device"] == 1
        assert a.debug_fastq_gzip_blocks() == (c0[0], c0[1] + 1, c0[2] + 1, c0[3])
        assert fc.batches_differ(a.fetch_reads(), outcome[1]) is None and st.stream_offset == len(f.stream)
    else:   # not FASTQ: the host inflater's bytes reach the host parser, whose error it is
        outcome, path = fc.host_outcome(tmp_path, name, f.data)
        assert outcome[0] == "error"
        with pytest.raises(capi.ThermiteError) as e:
            a.upload_fastq_gzip(st, f.stream, path=path)
        assert (e.value.code, fc.message(e.value)) == (outcome[1], outcome[2]) and e.value.code == capi.ERR_FORMAT
        assert st.key() == capi.GzipState().key()       # on any error the state is unchanged


@pytest.mark.parametrize("first,then", [(0, 0), (7000, 20000)])
@pytest.mark.parametrize("name", list(_CORRUPT))
def test_corrupt_streams_end_with_the_host_inflaters_error_at_the_same_call(name, first, then, tmp_path):
    stream = _CORRUPT[name][0]
    a = _world("test_ref").a
    want = _host_calls(stream, first, then)
    assert isinstance(want[-1], capi.ThermiteError) and want[-1].code == capi.ERR_IO
    st, at, size, head, k = capi.GzipState(), 0, first or len(stream), b"", 0
    path = str(tmp_path / (name + ".fastq.gz"))
    while True:
        n = min(size, len(stream) - at)
        last = at + n == len(stream)
        before = st.key()
        if isinstance(want[k], capi.ThermiteError):
            with pytest.raises(capi.ThermiteError) as e:
                a.upload_fastq_gzip(st, stream[at: at + n], head=head, path=path, last_block=last)
            assert e.value.code == capi.ERR_IO and _message(e.value) == _message(want[k]) and path in str(e.value)
            assert st.key() == before
            return
        info = a.upload_fastq_gzip(st, stream[at: at + n], head=head, path=path, last_block=last)
        assert (info["n_inflated_bytes"], info["n_consumed_bytes"]) == want[k], (name, k)
        head, at, k = info["tail"], at + info["n_consumed_bytes"], k + 1
        assert not last
        size = size * 2 if info["n_consumed_bytes"] == 0 else (then or len(stream))


@pytest.mark.parametrize("name", ["blank_tail_last", "bad_1_after_records", "quality_one_short_of_9000"])
def test_a_block_the_parser_declines_is_parsed_on_the_host_from_the_device_bytes(name, tmp_path):
    block, last, ref = fc.declined()[name]
    a = _world("test_ref").a
    outcome, path = fc.host_outcome(tmp_path, name, ref)
    c0 = a.debug_fastq_gzip_blocks()
    st = capi.GzipState()
    if outcome[0] == "batch":
        info = a.upload_fastq_gzip(st, gc.member(block), path=path, last_block=last)
        assert info["inflated_on_device"] == 1 and info["parsed_on_device"] == 0 and info["parse_ms"] == 0
        assert fc.batches_differ(a.fetch_reads(), outcome[1]) is None
        assert a.debug_fastq_gzip_blocks() == (c0[0] + 1, c0[1], c0[2], c0[3] + 1)
    else:
        with pytest.raises(capi.ThermiteError) as e:
            a.upload_fastq_gzip(st, gc.member(block), path=path, last_block=last)
        assert (e.value.code, fc.message(e.value)) == (outcome[1], outcome[2]) and e.value.code == capi.ERR_FORMAT
        assert st.key() == capi.GzipState().key()


# ------------------------------------------------------------------ 4. the run behind the upload
@pytest.mark.parametrize("name", ["test_query", "syn"])
def test_the_run_is_the_same_after_either_upload(name, tmp_path):
    w, rs = _set(name)
    text = fc.fastq_text(rs)
    outcome, path = fc.host_outcome(tmp_path, name, text)
    assert outcome[0] == "batch" and fc.batches_differ(outcome[1], bc.batch_of(rs)) is None
    a = w.aligner(rs["opts"])
    a.upload_reads(outcome[1])
    want = _run_both_fetches(a)
    d0, z0 = a.debug_fastq_device_blocks(), a.debug_fastq_bgzf_blocks()
    info = a.upload_fastq_gzip(capi.GzipState(), gzip.compress(text, 6, mtime=0), path=path)
    assert info["inflated_on_device"] == 1 and info["parsed_on_device"] == 1 and info["n_reads"] == len(rs["seqs"])
    assert a.debug_fastq_device_blocks() == d0 and a.debug_fastq_bgzf_blocks() == z0   # the existing calls' counters are their own
    _same_results(_run_both_fetches(a), want)
    assert want[1].n_failed == 0 and len(want[1].alns) > 0
    a.close()


# ------------------------------------------------------------------ 5. one aligner, one upload after the other; two aligners
def test_uploads_of_every_kind_in_a_row_leave_nothing_stale(tmp_path):
    import inflate_common as ic
    w = _world("test_ref")
    a = w.aligner(capi.CI_OPTS)
    ref = w.aligner(capi.CI_OPTS)
    other = bc.batch_of(dict(names=[b"u%d c" % i for i in range(9)], seqs=[b"ACGTTGCA" * (i + 1) for i in range(9)],
                             quals=[b"F" * (8 * (i + 1)) for i in range(9)]))
    plain = fc.well_formed()["lengths_62_66_126_130"]
    small = gc.text(42)
    for step, what in enumerate(("gzip", "bgzf", "plain", "gzip_host", "reads", "gzip")):
        if what == "reads":
            a.upload_reads(other)
            want = other
        elif what == "plain":
            outcome, path = fc.host_outcome(tmp_path, what, plain)
            want = outcome[1]
            assert a.upload_fastq(plain, path=path)["on_device"] == 1
        elif what == "bgzf":
            outcome, path = fc.host_outcome(tmp_path, what, small)
            want = outcome[1]
            assert a.upload_fastq_bgzf(ic.members_of(small, 1000), path=path)["inflated_on_device"] == 1
        elif what == "gzip_host":
            f = _DECLINED["fastq_over_the_ratio_cap"][0]
            outcome, path = fc.host_outcome(tmp_path, what, f.data)
            want = outcome[1]
            assert a.upload_fastq_gzip(capi.GzipState(), f.stream, path=path)["inflated_on_device"] == 0
        else:
            f = _WELL["three_members" if step else "empty_member"]
            outcome, path = fc.host_outcome(tmp_path, what, f.data)
            want = outcome[1]
            info = a.upload_fastq_gzip(capi.GzipState(), f.stream, path=path)
            assert info["inflated_on_device"] == 1 and info["parsed_on_device"] == 1
        assert fc.batches_differ(a.fetch_reads(), want) is None, (step, what)
        ref.upload_reads(want)
        _same_results(_run_both_fetches(a), _run_both_fetches(ref))
        assert fc.batches_differ(a.fetch_reads(), want) is None, (step, what)
    a.close()
    ref.close()


def test_state_and_tail_pass_between_two_aligners_on_one_device(tmp_path):
    w = _world("test_ref")
    a, b = w.aligner(capi.CI_OPTS), w.aligner(capi.CI_OPTS)
    f = _WELL["three_members"]
    outcome, path = fc.host_outcome(tmp_path, "two", f.data)
    infos, batches, st = _chain(None, f.stream, path, 40000, 40000, aligners=[a, b])
    assert len(infos) >= 4 and fc.batches_differ(_concat(batches), outcome[1]) is None
    assert all(i["inflated_on_device"] == 1 for i in infos) and st.n_members_done == 3
    assert a.debug_fastq_gzip_blocks()[0] + b.debug_fastq_gzip_blocks()[0] == len(infos)
    a.close()
    b.close()


# ------------------------------------------------------------------ 6. the file driver
N_DRIVER_READS = 294


@pytest.mark.parametrize("bam_device", ["1", "2"])
@pytest.mark.parametrize("batch_reads", [7, 1000])
def test_file_driver_with_the_gzip_inflater(bam_device, batch_reads, tmp_path, monkeypatch):
    """align_files to BAM with THM_BAM_DEVICE = 1 / 2, THM_FASTQ_DEVICE unset against 3, on plain-gzip files: the inflated
    BAM streams are the same, the counts are equal and the slices are inflated on the device.  BGZF, FASTA and plain input
    move no gzip counter."""
    import inflate_common as ic
    w, rs = _set("syn")
    sub = dict(names=rs["names"][:N_DRIVER_READS], seqs=rs["seqs"][:N_DRIVER_READS], quals=rs["quals"][:N_DRIVER_READS])
    text = fc.fastq_text(sub)
    fasta = b"".join(b">" + n + b"\n" + s + b"\n" for n, s in zip(sub["names"], sub["seqs"]))
    recs = text.split(b"\n@")
    third = [b"\n@".join(recs[:100]) + b"\n", b"@" + b"\n@".join(recs[100:200]) + b"\n", b"@" + b"\n@".join(recs[200:])]
    assert b"".join(third) == text
    eligible = {"level6.fastq.gz": gc.member(text), "mem_level1.fastq.gz": gc.member(text, 6, mem_level=1),
                "three_members.fastq.gz": gc.member(third[0], fname=b"a.fastq") + gc.member(third[1], 9, fhcrc=True) + gc.member(third[2], 1),
                "crlf.fastq.gz": gc.member(fc.fastq_text(sub, b"\r\n")), "blank_tail.fastq.gz": gc.member(text + b"\n\n")}
    other = {"bgzf.fastq.gz": ic.members_of(text, 512) + ic.EOF_BLOCK, "fasta.fa.gz": gc.member(fasta), "plain.fastq": text}
    for k, v in list(eligible.items()) + list(other.items()):
        (tmp_path / k).write_bytes(v)
    a = w.aligner(rs["opts"])
    monkeypatch.setenv("THM_BAM_DEVICE", bam_device)

    def run(al, paths, switch, tag):
        if switch:
            monkeypatch.setenv("THM_FASTQ_DEVICE", "3")
        else:
            monkeypatch.delenv("THM_FASTQ_DEVICE", raising=False)
        als = al if isinstance(al, list) else [al]
        before = [x.debug_fastq_gzip_blocks() for x in als]
        out = tmp_path / ("%s.%s.out" % ("+".join(paths), tag))
        st = capi.align_files(al, [tmp_path / p for p in paths], out, capi.FMT_BAM, batch_reads=batch_reads, n_threads=4)
        after = [x.debug_fastq_gzip_blocks() for x in als]
        moved = tuple(sum(y[k] - x[k] for x, y in zip(before, after)) for k in range(4))
        return out.read_bytes(), st, moved

    for paths in [[k] for k in eligible] + [["level6.fastq.gz", "mem_level1.fastq.gz"]]:
        off, st0, moved0 = run(a, paths, False, "off")
        on, st1, moved1 = run(a, paths, True, "on")
        assert gzip.decompress(on) == gzip.decompress(off), paths
        assert moved0 == (0, 0, 0, 0)
        assert moved1[0] >= len(paths) and moved1[1] == 0 and moved1[2] + moved1[3] >= len(paths), (paths, moved1)
        for k in ("n_reads", "n_aligned_reads", "n_records"):
            assert st0[k] == st1[k], (paths, k)
        assert st1["n_reads"] == N_DRIVER_READS * len(paths)
    for name in other:
        off, st0, _ = run(a, [name], False, "off")
        on, st1, moved = run(a, [name], True, "on")
        assert gzip.decompress(on) == gzip.decompress(off) and moved == (0, 0, 0, 0), name
        assert st0["n_reads"] == st1["n_reads"] == N_DRIVER_READS
    # a plain-gzip file between a BGZF file and a FASTA, and two aligners on one device
    b = w.aligner(rs["opts"])
    mixed = ["bgzf.fastq.gz", "level6.fastq.gz", "fasta.fa.gz", "three_members.fastq.gz"]
    off, st0, _ = run(a, mixed, False, "off2")
    on, st1, moved = run([a, b], mixed, True, "on2")
    assert gzip.decompress(on) == gzip.decompress(off)
    assert st0["n_reads"] == st1["n_reads"] == 4 * N_DRIVER_READS and st0["n_records"] == st1["n_records"]
    assert moved[0] >= 2 and moved[1] == 0
    # a malformed record in a plain-gzip file: the host parser's code and message
    bad = [b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in zip(sub["names"], sub["seqs"], sub["quals"])]
    bad[100] = b"@short quality\n" + sub["seqs"][100] + b"\n+\n" + sub["quals"][100][:-1] + b"\n"
    (tmp_path / "bad.fastq.gz").write_bytes(gc.member(b"".join(bad)))
    errs = []
    for switch in (False, True):
        with pytest.raises(capi.ThermiteError) as e:
            run(a, ["bad.fastq.gz"], switch, "bad")
        errs.append((e.value.code, str(e.value)))
    assert errs[0] == errs[1] and errs[0][0] == capi.ERR_FORMAT and "bad.fastq.gz:401" in errs[0][1], errs
    a.close()
    b.close()
