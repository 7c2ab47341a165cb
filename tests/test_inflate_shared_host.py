"""The DEFLATE block decoder that the device BGZF inflater and the device gzip inflater share (inf::decode_block of
thermite_amd/csrc/inflate_device.h, with the member sink there and the ring sink of gzip_device.h): one corrupt stream
through both sinks ends with one verdict.  The streams are the block-level corrupt fixtures of inflate_common.corrupt()
-- what is wrong with them is wrong inside a block, so both formats must name it alike; the remaining fixtures are wrong
in CRC, ISIZE or where the stream ends, which the two formats judge in different places.  A BGZF member is a gzip member
with an extra field, so the gzip model takes the same bytes."""
import pytest

import gzip_common as gc
import inflate_common as ic
import test_inflate_device_host as bgzf

BLOCK_LEVEL = ["block_type_3", "oversubscribed_code_lengths", "repeat_with_nothing_before_it", "literal_length_symbol_286",
               "distance_code_30", "distance_beyond_the_bytes_produced", "len_nlen_mismatch"]
WORDS = [ic.BLOCK_TYPE, ic.CODE_LENGTHS, ic.CODE_LENGTHS, ic.BAD_CODE, ic.BAD_CODE, ic.DISTANCE, ic.STORED_LEN]
CHUNKS = (64, 4096, gc.DEFAULT_CHUNK)


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    """name -> (the BGZF model's outcome, the gzip model's calls at every chunk size)"""
    tmp = tmp_path_factory.mktemp("inflate_shared")
    member = bgzf._run_all(bgzf._build(tmp, False), tmp, 0)
    exe = gc.build_model(tmp)
    inputs = [(name, ic.corrupt()[name][0]) for name in BLOCK_LEVEL]
    runs = {chunk: gc.run_model(exe, tmp, chunk, 0, inputs, last=1) for chunk in CHUNKS}
    return {name: (member[name], {chunk: runs[chunk][name].calls for chunk in CHUNKS}) for name in BLOCK_LEVEL}


@pytest.mark.parametrize("name,word", list(zip(BLOCK_LEVEL, WORDS)))
def test_one_stream_through_both_sinks_ends_with_one_verdict(verdicts, name, word):
    assert ic.corrupt()[name][1] == {word}                      # the single word the fixture names
    member, calls = verdicts[name]
    assert member[:3] == ("declined", 0, word), member
    for chunk in CHUNKS:
        assert [c.status for c in calls[chunk]] == [word], (chunk, calls[chunk])
