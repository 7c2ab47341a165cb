"""-m gpu: FASTQ blocks parsed on the device (kernels_fastq.hip, thm_batch_upload_fastq, thm_batch_fetch_reads, and the
file driver's THM_FASTQ_DEVICE=1).  The reference throughout is the host block parser, fastq_parse_block, reached
through FastqReader.all_by_blocks (tests/fastq_device_common.py): the batch it makes of the bytes, or its error."""
import gzip

import numpy as np
import pytest

import bam_common as bc
import fastq_device_common as fc
from gpu_common import World
from thermite_amd import capi

pytestmark = pytest.mark.gpu

_worlds, _sets = {}, {}
_WELL, _DECLINED = fc.well_formed(), fc.declined()


def _world(key):
    if key not in _worlds:
        _worlds[key] = World(bc.tables(key))
    return _worlds[key]


def _set(name):
    w = _world(bc.REF_OF[name])
    if name not in _sets:
        _sets[name] = bc.read_set(name, w.t)
    return w, _sets[name]


def _run_both_fetches(a):
    a.run()
    return a.fetch_bam(), a.fetch()


def _same_results(got, want):
    (gb, gr), (wb, wr) = got, want
    assert gb.data.tobytes() == wb.data.tobytes() and np.array_equal(gb.read_rec_off, wb.read_rec_off) and gb.n_records == wb.n_records
    assert np.array_equal(gr.offsets, wr.offsets) and np.array_equal(gr.alns, wr.alns) and np.array_equal(gr.ops, wr.ops)
    for g, w in ((gb, wb), (gr, wr)):
        assert g.n_failed == w.n_failed and (g.status is None) == (w.status is None)
        assert g.status is None or np.array_equal(g.status, w.status)


# ------------------------------------------------------------------ 1. blocks the device must take
@pytest.mark.parametrize("name", list(_WELL))
def test_well_formed_blocks_are_parsed_on_the_device(name, tmp_path):
    data = _WELL[name]
    a = _world("test_ref").a
    outcome, path = fc.host_outcome(tmp_path, name, data)
    assert outcome[0] == "batch"
    want = outcome[1]
    d0, h0 = a.debug_fastq_device_blocks()
    info = a.upload_fastq(data, path=path)
    print(name, len(data), "bytes", info)
    assert info["on_device"] == 1 and info["device_ms"] > 0
    assert a.debug_fastq_device_blocks() == (d0 + 1, h0)
    got = a.fetch_reads()
    assert fc.batches_differ(got, want) is None, fc.batches_differ(got, want)
    assert (info["n_reads"], info["n_bases"], info["n_name_bytes"]) == (len(want["offsets"]) - 1, len(want["bases"]), len(want["names"]))
    if name == "long_read":   # parsed like any other; the run refuses that one read, as it does after upload_reads
        got_run = _run_both_fetches(a)
        assert got_run[1].n_failed == 1 and got_run[1].status[fc.LONG_READ_INDEX] == capi.ERR_UNSUPPORTED
        assert got_run[0].status[fc.LONG_READ_INDEX] == capi.ERR_UNSUPPORTED
        a.upload_reads(want)
        _same_results(got_run, _run_both_fetches(a))


# ------------------------------------------------------------------ 2. the run behind either upload
@pytest.mark.parametrize("name", ["test_query", "syn"])
def test_the_run_is_the_same_after_either_upload(name, tmp_path):
    """the read set written out as FASTQ text (syn: lowercase, N, comments in the names): upload_fastq + run + fetch_bam /
    fetch against upload_reads of the host-parsed text + the same"""
    w, rs = _set(name)
    text = fc.fastq_text(rs)
    outcome, path = fc.host_outcome(tmp_path, name, text)
    assert outcome[0] == "batch" and fc.batches_differ(outcome[1], bc.batch_of(rs)) is None
    a = w.aligner(rs["opts"])
    a.upload_reads(outcome[1])
    want = _run_both_fetches(a)
    info = a.upload_fastq(text, path=path)
    assert info["on_device"] == 1 and info["n_reads"] == len(rs["seqs"])
    got = _run_both_fetches(a)
    _same_results(got, want)
    assert want[1].n_failed == 0 and len(want[1].alns) > 0
    a.close()


# ------------------------------------------------------------------ 3. blocks the device must decline
@pytest.mark.parametrize("name", list(_DECLINED))
def test_declined_blocks_end_as_the_host_parser_ends_them(name, tmp_path):
    block, last, ref = _DECLINED[name]
    a = _world("test_ref").a
    outcome, path = fc.host_outcome(tmp_path, name, ref)
    d0, h0 = a.debug_fastq_device_blocks()
    if outcome[0] == "batch":
        info = a.upload_fastq(block, path=path, last_block=last)
        assert info["on_device"] == 0 and info["device_ms"] == 0
        got = a.fetch_reads()
        assert fc.batches_differ(got, outcome[1]) is None, fc.batches_differ(got, outcome[1])
        assert info["n_reads"] == len(outcome[1]["offsets"]) - 1
    else:
        with pytest.raises(capi.ThermiteError) as e:
            a.upload_fastq(block, path=path, last_block=last)
        assert (e.value.code, fc.message(e.value)) == (outcome[1], outcome[2])
        assert e.value.code == capi.ERR_FORMAT
    assert a.debug_fastq_device_blocks() == (d0, h0 + 1)


# ------------------------------------------------------------------ 4. one aligner, one upload after the other
def test_uploads_in_a_row_leave_nothing_stale(tmp_path):
    """a large block, a small one, upload_reads, upload_fastq again: the buffers shrink and change hands, every batch is
    right, and so is the run behind each"""
    w = _world("test_ref")
    a = w.aligner(capi.CI_OPTS)
    ref = w.aligner(capi.CI_OPTS)
    other = bc.batch_of(dict(names=[b"u%d c" % i for i in range(9)], seqs=[b"ACGTTGCA" * (i + 1) for i in range(9)],
                             quals=[b"F" * (8 * (i + 1)) for i in range(9)]))
    for step, name in enumerate(("random", "one_record", None, "lengths_62_66_126_130", "crlf", "empty_read_in_the_middle")):
        if name is None:
            a.upload_reads(other)
            want = other
        else:
            outcome, path = fc.host_outcome(tmp_path, name, _WELL[name])
            want = outcome[1]
            assert a.upload_fastq(_WELL[name], path=path)["on_device"] == 1
        assert fc.batches_differ(a.fetch_reads(), want) is None, (step, name)
        ref.upload_reads(want)
        _same_results(_run_both_fetches(a), _run_both_fetches(ref))
        assert fc.batches_differ(a.fetch_reads(), want) is None, (step, name)   # the run leaves the batch alone
    a.close()
    ref.close()


def test_empty_input_and_a_batch_without_names():
    a = _world("test_ref").a
    info = a.upload_fastq(b"")
    assert (info["n_reads"], info["n_bases"], info["n_name_bytes"], info["on_device"]) == (0, 0, 0, 0)
    got = a.fetch_reads()
    assert len(got["offsets"]) == 1 and len(got["bases"]) == 0 and len(got["names"]) == 0
    a.upload(np.frombuffer(b"ACGTACGT", np.uint8), np.array([0, 8], "<u8"))   # plain upload: no names
    with pytest.raises(capi.ThermiteError) as e:
        a.fetch_reads()
    assert e.value.code == capi.ERR_INVALID_ARG
    b = bc.batch_of(dict(names=[b"n"], seqs=[b"ACGT"], quals=None))
    a.upload_reads(b)
    assert a.fetch_reads()["quals"] is None and fc.batches_differ(a.fetch_reads(), b) is None


# ------------------------------------------------------------------ 5. the file driver
N_DRIVER_READS = 294   # a multiple of 7: with batch_reads = 7 the blank tail is cut into a block of its own


@pytest.mark.parametrize("bam_device", ["1", "2"])
@pytest.mark.parametrize("batch_reads", [7, 1000])
def test_file_driver_with_the_device_parser(bam_device, batch_reads, tmp_path, monkeypatch):
    """align_files to BAM with THM_BAM_DEVICE = 1 / 2, THM_FASTQ_DEVICE unset against 1: the files are the same byte for
    byte, every block is parsed on the device except the one that holds the blank tail, and a malformed file fails with
    the same code and message"""
    w, rs = _set("syn")
    sub = dict(names=rs["names"][:N_DRIVER_READS], seqs=rs["seqs"][:N_DRIVER_READS], quals=rs["quals"][:N_DRIVER_READS])
    text = fc.fastq_text(sub)
    files = {"plain.fastq": text, "zipped.fastq.gz": gzip.compress(text), "crlf.fastq": fc.fastq_text(sub, b"\r\n"),
             "blank_tail.fastq": text + b"\n\n"}
    for k, v in files.items():
        (tmp_path / k).write_bytes(v)
    inputs = [[k] for k in files] + [["plain.fastq", "zipped.fastq.gz"]]
    a = w.aligner(rs["opts"])
    monkeypatch.setenv("THM_BAM_DEVICE", bam_device)

    def run(paths, switch, tag, fmt=capi.FMT_BAM):
        if switch:
            monkeypatch.setenv("THM_FASTQ_DEVICE", "1")
        else:
            monkeypatch.delenv("THM_FASTQ_DEVICE", raising=False)
        before = a.debug_fastq_device_blocks()
        out = tmp_path / ("%s.%s.out" % ("+".join(paths), tag))
        st = capi.align_files(a, [tmp_path / p for p in paths], out, fmt, batch_reads=batch_reads, n_threads=4)
        after = a.debug_fastq_device_blocks()
        return out.read_bytes(), st, (after[0] - before[0], after[1] - before[1])

    for paths in inputs:
        off, st0, moved0 = run(paths, False, "off")
        on, st1, moved1 = run(paths, True, "on")
        assert on == off, paths
        assert moved0 == (0, 0)
        n_blocks = sum(-(-N_DRIVER_READS // batch_reads) for _ in paths)
        assert moved1 == ((n_blocks, 0) if paths != ["blank_tail.fastq"] else (n_blocks - (batch_reads != 7), 1)), (paths, moved1)
        for k in ("n_reads", "n_aligned_reads", "n_records", "n_batches", "n_output_bytes"):
            assert st0[k] == st1[k], (paths, k)
        assert st1["n_reads"] == N_DRIVER_READS * len(paths)
    # a malformed record in the middle: the same code and message either way
    recs = [b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in zip(sub["names"], sub["seqs"], sub["quals"])]
    recs[100] = b"@short quality\n" + sub["seqs"][100] + b"\n+\n" + sub["quals"][100][:-1] + b"\n"
    (tmp_path / "bad.fastq").write_bytes(b"".join(recs))
    errs = []
    for switch in (False, True):
        with pytest.raises(capi.ThermiteError) as e:
            run(["bad.fastq"], switch, "bad")
        errs.append((e.value.code, str(e.value)))
    assert errs[0] == errs[1] and errs[0][0] == capi.ERR_FORMAT and "bad.fastq:401" in errs[0][1], errs
    if (bam_device, batch_reads) == ("1", 1000):
        # the switch is honoured in the BAM-device modes only: a SAM run, and a BAM run on the host encoder, ignore it
        monkeypatch.delenv("THM_BAM_DEVICE")
        for fmt in (capi.FMT_SAM, capi.FMT_BAM):
            off, _, _ = run(["plain.fastq"], False, "ignored_off", fmt)
            on, _, moved = run(["plain.fastq"], True, "ignored_on", fmt)
            assert on == off and moved == (0, 0)
    a.close()
