"""-m gpu: THM_CELLS in the file driver (thm_align_files).  The output file must be the unset run's byte for byte; the three
files beside it must be what tests/cells_common.py computes from the records of the SAM output and the names in the FASTQ
file -- a way that goes through neither the oracle's alignments nor anything of thm_cells."""
import contextlib
import os

import pytest

import cells_common as cl
import quant_common as qc
from gpu_common import World
from thermite_amd import capi

pytestmark = pytest.mark.gpu

KNOBS = ("THM_CELLS", "THM_CELLS_CB_LEN", "THM_CELLS_UMI_LEN", "THM_CELLS_MIN_UMIS", "THM_QUANT", "THM_COVERAGE", "THM_PILEUP", "THM_BAM_SORT",
         "THM_BAM_INDEX", "THM_BAM_DEVICE", "THM_FASTQ_DEVICE")
SIDE = (".cells.mtx", ".cells.barcodes.tsv", ".cells.features.tsv")
_memo = {}


@contextlib.contextmanager
def _knobs(**kv):
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _raises(f):
    with pytest.raises(capi.ThermiteError) as e:
        f()
    return e.value


def _setup(tmp_path):
    if "w" not in _memo:
        _memo["w"] = World(qc.syn_tables())
    w = _memo["w"]
    bases, off = qc.syn_reads(w.t)
    n = len(off) - 1
    names = cl.gen_names(n, 2024)
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(b"".join(b"@" + names[i] + b"\n" + bytes(bases[int(off[i]): int(off[i + 1])]) + b"\n+\n" + b"I" * int(off[i + 1] - off[i]) + b"\n"
                            for i in range(n)))
    return w, fq, names


def _run(a, fq, tmp_path, tag, fmt, **knobs):
    out = tmp_path / tag
    with _knobs(**knobs):
        capi.align_files(a, [fq], out, fmt, batch_reads=700, n_threads=4)   # 700 does not divide 4000
    side = [tmp_path / (tag + s) for s in SIDE]
    return out.read_bytes(), tuple(p.read_text() for p in side) if all(p.exists() for p in side) else None


def test_file_driver_writes_the_matrix_and_leaves_the_output_alone(tmp_path):
    w, fq, names = _setup(tmp_path)
    a = w.aligner(capi.CI_OPTS)
    sam_plain, none = _run(a, fq, tmp_path, "sam_plain", capi.FMT_SAM)
    assert none is None and not any((tmp_path / ("sam_plain" + s)).exists() for s in SIDE)
    # the expectation: the SAM file's own records, and the names as the FASTQ file has them
    offsets, alns, _, _ = qc.sam_view(str(tmp_path / "sam_plain"), w.t)
    assert len(offsets) - 1 == len(names)
    pool, name_off = cl.join_names(names)
    want = {}
    for flags in (0, 1):
        mol, tot = cl.expected(w.t, offsets, alns, None, pool, name_off, flags, 16, 12)
        for min_umis in (1, 3):
            cells, entries, _ = cl.rows(mol, min_umis)
            want[(flags, min_umis)] = cl.mtx_of(w.t, cells, entries, 16)
    assert want[(0, 1)] != want[(1, 1)] and want[(0, 1)][0] != want[(0, 3)][0] and want[(0, 1)][0].count("\n") > 50
    bam_knobs = dict(THM_BAM_DEVICE=2, THM_FASTQ_DEVICE=1)
    bam_plain, none = _run(a, fq, tmp_path, "bam_plain", capi.FMT_BAM, **bam_knobs)
    assert none is None
    for value in (1, 2):
        got, files = _run(a, fq, tmp_path, "sam_cells%d" % value, capi.FMT_SAM, THM_CELLS=value)
        assert got == sam_plain and files == want[(value - 1, 1)], value
        got, files = _run(a, fq, tmp_path, "bam_cells%d" % value, capi.FMT_BAM, THM_CELLS=value, THM_CELLS_MIN_UMIS=3, **bam_knobs)
        assert got == bam_plain and files == want[(value - 1, 3)], value
    # other lengths: with 12 bases of barcode and 12 of UMI the tag is the last 26 bytes, whose first is a base of the
    # 16-base barcode and no '_' -- no read has a tag, and the matrix is empty
    got, files = _run(a, fq, tmp_path, "sam_short", capi.FMT_SAM, THM_CELLS=1, THM_CELLS_CB_LEN=12, THM_CELLS_UMI_LEN=12)
    mol, tot = cl.expected(w.t, offsets, alns, None, pool, name_off, 0, 12, 12)
    assert got == sam_plain and not mol and files == cl.mtx_of(w.t, *cl.rows(mol, 1)[:2], 12)
    # THM_CELLS=0 is the unset run
    got, files = _run(a, fq, tmp_path, "sam_zero", capi.FMT_SAM, THM_CELLS=0)
    assert got == sam_plain and files is None
    a.close()


def test_file_driver_refusals(tmp_path):
    w, fq, names = _setup(tmp_path)
    a, a2 = w.aligner(capi.CI_OPTS), w.aligner(capi.CI_OPTS)
    for knobs in (dict(THM_CELLS=3), dict(THM_CELLS="yes"), dict(THM_CELLS=1, THM_CELLS_CB_LEN=17), dict(THM_CELLS=1, THM_CELLS_UMI_LEN=0),
                  dict(THM_CELLS=1, THM_CELLS_MIN_UMIS=0), dict(THM_CELLS=1, THM_CELLS_CB_LEN="x")):
        with _knobs(**knobs):
            e = _raises(lambda: capi.align_files(a, [fq], tmp_path / "bad", capi.FMT_SAM, batch_reads=700, n_threads=4))
        assert e.code == capi.ERR_INVALID_ARG and "THM_CELLS" in str(e), knobs
    with _knobs(THM_CELLS=1):
        e = _raises(lambda: capi.align_files(a, [fq], "-", capi.FMT_SAM, batch_reads=700, n_threads=4))
        assert e.code == capi.ERR_INVALID_ARG and "THM_CELLS" in str(e) and "output file" in str(e)
        e = _raises(lambda: capi.align_files([a, a2], [fq], tmp_path / "two", capi.FMT_SAM, batch_reads=700, n_threads=4))
        assert e.code == capi.ERR_INVALID_ARG and "one aligner" in str(e) and "union" in str(e)
    assert not any((tmp_path / ("two" + s)).exists() for s in SIDE)
    a.close()
    a2.close()
