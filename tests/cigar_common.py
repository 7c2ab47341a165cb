"""What thm_aln_digest and the CIGAR word pool must hold, restated from the oracle alone: the op list comes from
oracle.pyoracle.decode_ops, the runs from oracle.aln_writer.to_cigar (to_noodles_cigar, reference
src/aln_writer.rs:279-323), the counts follow oracle.aln_writer.paf_record / sam_record (PafEntry::new :55-72, nM
:160-168).  Nothing here touches the library under test."""
import re

import numpy as np

from oracle import aln_writer as ow
from oracle import pyoracle as orc

LONG_RUN, MALFORMED = 1, 2          # THM_DIGEST_*, include/thermite.h
MAX_RUN = 1 << 28                   # a BAM CIGAR word holds 28 bits of length
BAM_CODE = {"M": 0, "I": 1, "D": 2, "N": 3, "S": 4}   # SAM specification, section 4.2
_RUN = re.compile(r"(\d+)([MIDNS])")

DIGEST_DT = np.dtype([("cigar_off", "<u8"), ("ref_len", "<u8"), ("n_cigar", "<u4"), ("n_tx_cigar", "<u4"),
                      ("n_match", "<u4"), ("n_subst", "<u4"), ("n_not_yclip", "<u4"), ("flags", "<u4")])


def cigar_runs(text):
    """'12M3N' -> [(12, 'M'), (3, 'N')]; '*' -> []"""
    if text == "*":
        return []
    runs = [(int(n), k) for n, k in _RUN.findall(text)]
    assert "".join("%d%s" % r for r in runs) == text, text
    return runs


def well_formed(stream):
    """a serialised op stream is well formed when the oracle's decoder and encoder round-trip it: a kind above 5 has
    no name, and a clip cut by the end of the stream comes back with all five of its bytes"""
    b = bytes(stream)
    try:
        return orc.encode_ops(orc.decode_ops(b)) == b
    except IndexError:
        return False


_cache = {}


def expected_stream(stream):
    """one op stream -> (words list, ref_len, n_match, n_subst, n_not_yclip, flags)"""
    b = bytes(stream)
    hit = _cache.get(b)
    if hit is not None:
        return hit
    try:
        ops = orc.decode_ops(b)
        ok = orc.encode_ops(ops) == b      # well_formed(b), with the op list kept
    except IndexError:
        ok = False
    if not ok:
        out = ([], 0, 0, 0, 0, MALFORMED)
    else:
        runs = cigar_runs(ow.to_cigar(ops))
        n_match = ops.count("Match")                                   # PafEntry::num_match
        n_subst = ops.count("Subst")                                   # nM
        n_yclip = sum(1 for o in ops if isinstance(o, tuple) and o[0] == "Yclip")
        ref_len = sum(n for n, k in runs if k in "MDN")
        long_run = any(n >= MAX_RUN for n, _ in runs)
        words = [] if long_run else [(n << 4) | BAM_CODE[k] for n, k in runs]
        out = (words, ref_len, n_match, n_subst, len(ops) - n_yclip, LONG_RUN if long_run else 0)
    if len(_cache) < 400000:
        _cache[b] = out
    return out


def expected_streams(streams):
    """streams (bytes-likes) -> (DIGEST_DT array, words array): what thm_cigar_encode_batch returns for them"""
    dig = np.zeros(len(streams), DIGEST_DT)
    words = []
    for i, s in enumerate(streams):
        w, ref_len, nm, ns, nny, flags = expected_stream(s)
        dig[i] = (len(words), ref_len, len(w), 0, nm, ns, nny, flags)
        words += w
    return dig, np.array(words, "<u4")


def expected_alignments(alns, ops):
    """ALN_DT records and their op pool (an oracle or a plain-fetch result) -> (DIGEST_DT array, words array): the
    genome CIGAR of every alignment, the transcript CIGAR of an exonic one directly behind it"""
    dig = np.zeros(len(alns), DIGEST_DT)
    words = []
    pool = bytes(ops)
    o0, l0, o1, l1, ty = (alns[f].tolist() for f in ("ops_off", "ops_len", "tx_ops_off", "tx_ops_len", "aln_type"))
    for i in range(len(alns)):
        w, ref_len, nm, ns, nny, flags = expected_stream(pool[o0[i]: o0[i] + l0[i]])
        tw, tflags = [], 0
        if ty[i] == 0:
            tw, _, _, _, _, tflags = expected_stream(pool[o1[i]: o1[i] + l1[i]])
        dig[i] = (len(words), ref_len, len(w), len(tw), nm, ns, nny, flags | (tflags << 8))
        words += w
        words += tw
    return dig, np.array(words, "<u4")


def assert_digests_equal(got_dig, got_words, exp_dig, exp_words, what=""):
    assert len(got_dig) == len(exp_dig), (what, len(got_dig), len(exp_dig))
    for f in DIGEST_DT.names:
        bad = np.nonzero(got_dig[f] != exp_dig[f])[0]
        assert len(bad) == 0, "%s digest field %s differs at %d: got %s expected %s" % (what, f, bad[0], got_dig[bad[0]], exp_dig[bad[0]])
    assert len(got_words) == len(exp_words), (what, len(got_words), len(exp_words))
    bad = np.nonzero(got_words != exp_words)[0]
    assert len(bad) == 0, "%s word %d differs: got %#x expected %#x" % (what, bad[0], got_words[bad[0]], exp_words[bad[0]])


def words_to_text(words):
    return "".join("%d%s" % (int(w) >> 4, "MIDNS"[int(w) & 15]) for w in words) or "*"


# ------------------------------------------------------------------ op streams for the operator-level tests
def clip(kind, n):
    return bytes([kind]) + int(n).to_bytes(4, "little")


def random_stream(rng, length, clip_density, malformed=False, long_clips=False):
    """a well-formed stream of about `length` bytes from a random.Random: plain ops in runs, clips with probability
    clip_density per token whose payload bytes take all byte values (4 and 5 among them); lengths stay below 2^28
    unless long_clips.  malformed=True: the same with a kind above 5 put at a token position, or cut inside its last
    clip."""
    top = (1 << 32) if long_clips else (1 << 28)
    out = bytearray()
    tokens = []  # offsets of token starts
    while len(out) < length:
        if rng.random() < clip_density:
            tokens.append(len(out))
            kind = 4 + rng.randrange(2)
            r = rng.random()
            if r < 0.2 and len(out) >= 5:   # the previous five bytes' length again: equal adjacent clips merge
                n = int.from_bytes(out[-4:], "little") % top
            elif r < 0.6:                   # bytes 4 and 5 frequent
                n = int.from_bytes(bytes(rng.choice((0, 1, 4, 5, 255)) for _ in range(4)), "little") % top
            else:
                n = rng.randrange(top)
            out += clip(kind, n)
        else:
            k = rng.randrange(4)
            run = 1 + rng.randrange(1 + rng.randrange(80)) if rng.random() < 0.5 else 1
            if k <= 1 and run > 2:          # Subst inside Match runs and the reverse
                body = bytearray([k]) * run
                for _ in range(1 + run // 10):
                    body[rng.randrange(run)] = 1 - k
            else:
                body = bytes([k]) * run
            tokens.extend(range(len(out), len(out) + run))
            out += body
    if malformed:
        clips = [t for t in tokens if out[t] >= 4]
        if clips and rng.random() < 0.5:
            del out[clips[-1] + 1 + rng.randrange(4):]   # the last clip keeps 0..3 payload bytes
        elif tokens:
            out[tokens[rng.randrange(len(tokens))]] = rng.randrange(6, 256)
        else:
            out.append(rng.randrange(6, 256))
    return bytes(out)
