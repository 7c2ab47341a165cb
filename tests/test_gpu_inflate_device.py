"""-m gpu: BGZF members inflated on the device (kernels_inflate.hip, thm_batch_upload_fastq_bgzf and its debug hooks).
The reference for the bytes is gzip.decompress; for batches and errors it is the host path -- GzInflater plus
fastq_parse_block, through FastqReader.all_by_blocks on the members written out as a file (tests/inflate_common.py).
Everything is byte equality."""
import gzip

import numpy as np
import pytest

import bam_common as bc
import fastq_device_common as fc
import inflate_common as ic
from gpu_common import World
from thermite_amd import capi

pytestmark = pytest.mark.gpu

_worlds, _sets = {}, {}
_WELL, _NOT, _CORRUPT = ic.well_formed(), ic.not_for_device(), ic.corrupt()
_FASTQ = [k for k, f in _WELL.items() if f.fastq]


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


def _concat(batches):
    """batches of consecutive reads as one"""
    out = {k: [] for k in fc.KEYS}
    nb = nn = 0
    for b in batches:
        out["names"].append(b["names"])
        out["bases"].append(b["bases"])
        out["quals"].append(b["quals"] if b["quals"] is not None else np.zeros(0, np.uint8))
        out["offsets"].append(np.asarray(b["offsets"][:-1], "<u8") + nb)
        out["name_off"].append(np.asarray(b["name_off"][:-1], "<u8") + nn)
        nb += int(b["offsets"][-1])
        nn += int(b["name_off"][-1])
    out["offsets"].append(np.array([nb], "<u8"))
    out["name_off"].append(np.array([nn], "<u8"))
    return {k: np.concatenate(v) for k, v in out.items()}


# ------------------------------------------------------------------ 1. the inflate alone: no host inflater behind it
@pytest.mark.parametrize("name", list(_WELL))
def test_every_well_formed_fixture_inflates_on_the_device(name):
    f = _WELL[name]
    a = _world("test_ref").a
    got = a.debug_bgzf_inflate(f.members, cap=len(f.data))
    assert got == f.data == gzip.decompress(f.members)


def test_the_projects_own_encoders_inflate_on_the_device():
    """the members thm_batch_fetch_bgzf makes of a small run, and a block from the host writer's deflate_block"""
    w, rs = _set("test_query")
    a = w.aligner(rs["opts"])
    a.upload_reads(bc.batch_of(rs))
    a.run()
    z, bam = a.fetch_bgzf(), a.fetch_bam()
    assert z.n_blocks >= 1
    assert a.debug_bgzf_inflate(z.data.tobytes(), cap=len(bam.data)) == bam.data.tobytes()
    text = ic.fastq_text(30000, 15)
    assert a.debug_bgzf_inflate(ic.frame(capi.debug_deflate_block(text), text), cap=len(text)) == text
    a.close()


@pytest.mark.parametrize("name", list(_NOT) + list(_CORRUPT))
def test_the_hook_has_no_fallback(name):
    """what the device does not take is an error of the hook, never bytes"""
    a = _world("test_ref").a
    members = _NOT[name].members if name in _NOT else _CORRUPT[name][0]
    with pytest.raises(capi.ThermiteError) as e:
        a.debug_bgzf_inflate(members, cap=1 << 20)
    assert e.value.code == capi.ERR_UNSUPPORTED
    if name in _CORRUPT and _CORRUPT[name][1] is not None:
        assert any(str(e.value).endswith("member 0 declined with status %d" % s) for s in _CORRUPT[name][1]), str(e.value)


# ------------------------------------------------------------------ 2. the call: inflate + parse, batch and tail
@pytest.mark.parametrize("name", _FASTQ)
def test_fastq_fixtures_are_inflated_and_parsed_on_the_device(name, tmp_path):
    f = _WELL[name]
    a = _world("test_ref").a
    outcome, path = fc.host_outcome(tmp_path, name, f.data)
    assert outcome[0] == "batch"
    want = outcome[1]
    c0 = a.debug_fastq_bgzf_blocks()
    info = a.upload_fastq_bgzf(f.members, path=path)
    print(name, len(f.members), "->", len(f.data), {k: v for k, v in info.items() if k != "tail"})
    assert info["inflated_on_device"] == 1 and info["parsed_on_device"] == 1 and info["inflate_ms"] > 0 and info["parse_ms"] > 0
    assert info["tail"] == b"" and info["tail_len"] == 0
    assert (info["n_members"], info["n_inflated_bytes"]) == (len(ic.split_members(f.members)), len(f.data))
    assert info["n_lines"] == 4 * info["n_reads"]
    c1 = a.debug_fastq_bgzf_blocks()
    assert c1 == (c0[0] + 1, c0[1], c0[2] + 1, c0[3])
    got = a.fetch_reads()
    assert fc.batches_differ(got, want) is None, fc.batches_differ(got, want)
    assert (info["n_reads"], info["n_bases"], info["n_name_bytes"]) == (len(want["offsets"]) - 1, len(want["bases"]), len(want["names"]))


@pytest.mark.parametrize("name", _FASTQ)
def test_a_chain_of_three_calls_gives_the_whole_text(name, tmp_path):
    """the members in three groups, each call's tail the head of the next, last_block on the third only: the batches
    together are the host parse of the whole text, every tail is the bytes behind its batch"""
    f = _WELL[name]
    a = _world("test_ref").a
    outcome, path = fc.host_outcome(tmp_path, name, f.data)
    want = outcome[1]
    ms = ic.split_members(f.members)
    k = len(ms)
    groups = [ms[: k // 3], ms[k // 3: 2 * k // 3], ms[2 * k // 3:]]
    head, line, batches, consumed, inflated = b"", 1, [], 0, b""
    zero_reads = 0
    for g, grp in enumerate(groups):
        members = b"".join(grp)
        info = a.upload_fastq_bgzf(members, head=head, path=path, first_line=line, last_block=(g == 2))
        inflated += b"".join(gzip.decompress(m) for m in grp)
        block = f.data[consumed: len(inflated)]
        assert info["inflated_on_device"] == (1 if grp else 0)
        if g == 2:
            cut = len(block)
        else:
            nl = block.count(b"\n")
            cut = 0 if nl < 4 else [i for i, c in enumerate(block) if c == 10][4 * (nl // 4) - 1] + 1
        assert info["tail"] == block[cut:], (g, len(info["tail"]), len(block) - cut)
        assert info["n_lines"] == block[:cut].count(b"\n") + (1 if cut and block[cut - 1] != 10 else 0)
        assert info["parsed_on_device"] == (1 if info["n_reads"] else 0)
        zero_reads += info["n_reads"] == 0
        batches.append(a.fetch_reads())
        assert len(batches[-1]["offsets"]) - 1 == info["n_reads"]
        head, line, consumed = info["tail"], line + info["n_lines"], consumed + cut
    got = _concat(batches)
    assert fc.batches_differ(got, want) is None, fc.batches_differ(got, want)
    if len(ms) == 1:
        assert zero_reads == 2   # the calls without members, and without a head, have no read


@pytest.mark.parametrize("head_len", [1, 3, 17])
def test_a_head_shifts_every_member_output(head_len, tmp_path):
    text = ic.fastq_text(9000, 31)
    a = _world("test_ref").a
    outcome, path = fc.host_outcome(tmp_path, "shift", text)
    info = a.upload_fastq_bgzf(ic.members_of(text[head_len:], 1000), head=text[:head_len], path=path)
    assert info["inflated_on_device"] == 1 and info["parsed_on_device"] == 1 and info["n_inflated_bytes"] == len(text) - head_len
    assert fc.batches_differ(a.fetch_reads(), outcome[1]) is None


def test_a_block_without_four_lines_is_all_tail():
    a = _world("test_ref").a
    text = b"@r1 x\nACGT\n+\n"
    info = a.upload_fastq_bgzf(ic.member(text[3:]), head=text[:3], last_block=False)
    assert (info["n_reads"], info["n_lines"], info["tail"], info["inflated_on_device"], info["parsed_on_device"]) == (0, 0, text, 1, 0)
    assert len(a.fetch_reads()["offsets"]) == 1
    info = a.upload_fastq_bgzf(b"", head=b"", last_block=True)
    assert (info["n_reads"], info["tail"], info["inflated_on_device"], info["n_members"]) == (0, b"", 0, 0)


# ------------------------------------------------------------------ 3. what the device does not take ends as the host ends it
@pytest.mark.parametrize("name", [k for k, f in _NOT.items() if f.fastq])
def test_valid_gzip_that_is_not_bgzf_is_inflated_on_the_host(name, tmp_path):
    f = _NOT[name]
    a = _world("test_ref").a
    outcome, path = ic.host_outcome_gz(tmp_path, name, f.members)
    assert outcome[0] == "batch"
    c0 = a.debug_fastq_bgzf_blocks()
    info = a.upload_fastq_bgzf(f.members, path=path)
    assert info["inflated_on_device"] == 0 and info["inflate_ms"] == 0 and info["parsed_on_device"] == 1
    assert info["n_inflated_bytes"] == len(f.data) and info["tail"] == b""
    assert a.debug_fastq_bgzf_blocks() == (c0[0], c0[1] + 1, c0[2] + 1, c0[3])
    assert fc.batches_differ(a.fetch_reads(), outcome[1]) is None


@pytest.mark.parametrize("name", list(_CORRUPT))
def test_corrupt_members_end_with_the_host_inflaters_error(name, tmp_path):
    members = _CORRUPT[name][0]
    a = _world("test_ref").a
    outcome, path = ic.host_outcome_gz(tmp_path, name, members)
    assert outcome[0] == "error" and outcome[1] == capi.ERR_IO
    c0 = a.debug_fastq_bgzf_blocks()
    with pytest.raises(capi.ThermiteError) as e:
        a.upload_fastq_bgzf(members, path=path)
    assert (e.value.code, fc.message(e.value)) == (outcome[1], outcome[2])
    assert a.debug_fastq_bgzf_blocks() == c0     # neither inflated nor parsed: the call failed


def test_a_corrupt_member_among_good_ones_declines_the_whole_inflate(tmp_path):
    text = ic.fastq_text(6000, 33)
    good = ic.split_members(ic.members_of(text, 1500))
    bad = _CORRUPT["crc_flipped"][0]
    a = _world("test_ref").a
    members = b"".join(good[:2]) + bad + b"".join(good[2:])
    outcome, path = ic.host_outcome_gz(tmp_path, "mixed", members)
    with pytest.raises(capi.ThermiteError) as e:
        a.upload_fastq_bgzf(members, path=path)
    assert (e.value.code, fc.message(e.value)) == (outcome[1], outcome[2]) and e.value.code == capi.ERR_IO


@pytest.mark.parametrize("name", ["blank_tail_last", "bad_1_after_records", "quality_one_short_of_9000"])
def test_a_block_the_parser_declines_is_parsed_on_the_host_from_the_device_bytes(name, tmp_path):
    """inflated on the device, declined by the device parser: the bytes come down and the host parser has the last word"""
    block, last, ref = fc.declined()[name]
    a = _world("test_ref").a
    outcome, path = fc.host_outcome(tmp_path, name, ref)
    c0 = a.debug_fastq_bgzf_blocks()
    members = ic.members_of(block, 777)
    if outcome[0] == "batch":
        info = a.upload_fastq_bgzf(members, path=path, last_block=last)
        assert info["inflated_on_device"] == 1 and info["parsed_on_device"] == 0 and info["parse_ms"] == 0
        assert fc.batches_differ(a.fetch_reads(), outcome[1]) is None
        assert a.debug_fastq_bgzf_blocks() == (c0[0] + 1, c0[1], c0[2], c0[3] + 1)
    else:
        with pytest.raises(capi.ThermiteError) as e:
            a.upload_fastq_bgzf(members, path=path, last_block=last)
        assert (e.value.code, fc.message(e.value)) == (outcome[1], outcome[2]) and e.value.code == capi.ERR_FORMAT


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
    d0 = a.debug_fastq_device_blocks()
    info = a.upload_fastq_bgzf(ic.members_of(text, 0xff00), path=path)
    assert info["inflated_on_device"] == 1 and info["parsed_on_device"] == 1 and info["n_reads"] == len(rs["seqs"])
    assert a.debug_fastq_device_blocks() == d0     # the existing call's counters are its own
    got = _run_both_fetches(a)
    _same_results(got, want)
    assert want[1].n_failed == 0 and len(want[1].alns) > 0
    a.close()


# ------------------------------------------------------------------ 5. one aligner, one upload after the other
def test_uploads_in_a_row_leave_nothing_stale(tmp_path):
    w = _world("test_ref")
    a = w.aligner(capi.CI_OPTS)
    ref = w.aligner(capi.CI_OPTS)
    other = bc.batch_of(dict(names=[b"u%d c" % i for i in range(9)], seqs=[b"ACGTTGCA" * (i + 1) for i in range(9)],
                             quals=[b"F" * (8 * (i + 1)) for i in range(9)]))
    plain = fc.well_formed()["lengths_62_66_126_130"]
    for step, what in enumerate(("dynamic_fastq_level_6", "one_byte_members_40", "plain", "reads", "cut_every_100", "isize_65536")):
        if what == "reads":
            a.upload_reads(other)
            want = other
        elif what == "plain":
            outcome, path = fc.host_outcome(tmp_path, what, plain)
            want = outcome[1]
            assert a.upload_fastq(plain, path=path)["on_device"] == 1
        else:
            outcome, path = fc.host_outcome(tmp_path, what, _WELL[what].data)
            want = outcome[1]
            info = a.upload_fastq_bgzf(_WELL[what].members, path=path)
            assert info["inflated_on_device"] == 1 and info["parsed_on_device"] == 1
        assert fc.batches_differ(a.fetch_reads(), want) is None, (step, what)
        ref.upload_reads(want)
        _same_results(_run_both_fetches(a), _run_both_fetches(ref))
        assert fc.batches_differ(a.fetch_reads(), want) is None, (step, what)
    a.close()
    ref.close()


# ------------------------------------------------------------------ 6. the file driver
N_DRIVER_READS = 294


@pytest.mark.parametrize("bam_device", ["1", "2"])
@pytest.mark.parametrize("batch_reads", [7, 1000])
def test_file_driver_with_the_device_inflater(bam_device, batch_reads, tmp_path, monkeypatch):
    """align_files to BAM with THM_BAM_DEVICE = 1 / 2, THM_FASTQ_DEVICE unset against 2, on BGZF files of 512-byte members:
    the inflated BAM streams are the same (batch boundaries differ, so the compressed bytes may), the counts are equal,
    and every group is inflated on the device.  Inputs that are not BGZF FASTQ throughout give the very file they give
    with the switch unset and move none of the new counters."""
    w, rs = _set("syn")
    sub = dict(names=rs["names"][:N_DRIVER_READS], seqs=rs["seqs"][:N_DRIVER_READS], quals=rs["quals"][:N_DRIVER_READS])
    text = fc.fastq_text(sub)
    fasta = b"".join(b">" + n + b"\n" + s + b"\n" for n, s in zip(sub["names"], sub["seqs"]))
    eligible = {"bgzf.fastq.gz": ic.members_of(text, 512) + ic.EOF_BLOCK, "crlf.fastq.gz": ic.members_of(fc.fastq_text(sub, b"\r\n"), 512),
                "blank_tail.fastq.gz": ic.members_of(text + b"\n\n", 512) + ic.EOF_BLOCK}
    other = {"plain_gzip.fastq.gz": gzip.compress(text, mtime=0), "bgzf_fasta.fa.gz": ic.members_of(fasta, 512),
             "trailing_garbage.fastq.gz": ic.members_of(text, 512) + b"not a member"}
    for k, v in list(eligible.items()) + list(other.items()):
        (tmp_path / k).write_bytes(v)
    a = w.aligner(rs["opts"])
    monkeypatch.setenv("THM_BAM_DEVICE", bam_device)

    def run(al, paths, switch, tag):
        if switch:
            monkeypatch.setenv("THM_FASTQ_DEVICE", "2")
        else:
            monkeypatch.delenv("THM_FASTQ_DEVICE", raising=False)
        als = al if isinstance(al, list) else [al]
        before = [x.debug_fastq_bgzf_blocks() for x in als]
        out = tmp_path / ("%s.%s.out" % ("+".join(paths), tag))
        st = capi.align_files(al, [tmp_path / p for p in paths], out, capi.FMT_BAM, batch_reads=batch_reads, n_threads=4)
        after = [x.debug_fastq_bgzf_blocks() for x in als]
        moved = tuple(sum(y[k] - x[k] for x, y in zip(before, after)) for k in range(4))
        return out.read_bytes(), st, moved

    for paths in [[k] for k in eligible] + [["bgzf.fastq.gz", "crlf.fastq.gz"]]:
        off, st0, moved0 = run(a, paths, False, "off")
        on, st1, moved1 = run(a, paths, True, "on")
        assert gzip.decompress(on) == gzip.decompress(off), paths
        assert moved0 == (0, 0, 0, 0)
        assert moved1[0] >= len(paths) and moved1[1] == 0 and moved1[2] + moved1[3] >= len(paths), (paths, moved1)
        assert moved1[3] == (1 if paths == ["blank_tail.fastq.gz"] else 0), (paths, moved1)   # the block with the blank tail
        for k in ("n_reads", "n_aligned_reads", "n_records"):
            assert st0[k] == st1[k], (paths, k)
        assert st1["n_reads"] == N_DRIVER_READS * len(paths)
        if batch_reads == 7:
            assert st1["n_batches"] > 10 * len(paths)
    for name in other:
        off, st0, _ = run(a, [name], False, "off")
        on, st1, moved = run(a, [name], True, "on")
        assert on == off and moved == (0, 0, 0, 0), name
        assert st0["n_reads"] == st1["n_reads"] == N_DRIVER_READS
    # an eligible file beside one that is not, and two aligners on one device
    b = w.aligner(rs["opts"])
    mixed = ["bgzf.fastq.gz", "plain_gzip.fastq.gz", "crlf.fastq.gz"]
    off, st0, _ = run(a, mixed, False, "off2")
    on, st1, moved = run([a, b], mixed, True, "on2")
    assert gzip.decompress(on) == gzip.decompress(off)
    assert st0["n_reads"] == st1["n_reads"] == 3 * N_DRIVER_READS and st0["n_records"] == st1["n_records"]
    assert moved[0] >= 2 and moved[1] == 0
    # a malformed record in a BGZF file: the host parser's code and message
    recs = [b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n" for n, s, q in zip(sub["names"], sub["seqs"], sub["quals"])]
    recs[100] = b"@short quality\n" + sub["seqs"][100] + b"\n+\n" + sub["quals"][100][:-1] + b"\n"
    (tmp_path / "bad.fastq.gz").write_bytes(ic.members_of(b"".join(recs), 512))
    errs = []
    for switch in (False, True):
        with pytest.raises(capi.ThermiteError) as e:
            run(a, ["bad.fastq.gz"], switch, "bad")
        errs.append((e.value.code, str(e.value)))
    assert errs[0] == errs[1] and errs[0][0] == capi.ERR_FORMAT and "bad.fastq.gz:401" in errs[0][1], errs
    a.close()
    b.close()
