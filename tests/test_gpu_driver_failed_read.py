"""-m gpu: the whole-file driver names a read it cannot take, whichever way the block went up.  The file of
test_gpu_files.test_align_files_reports_errors -- one 12-base read, then `@giant read` of 68 000 bases -- to BAM with
THM_BAM_DEVICE=1 and THM_FASTQ_DEVICE unset, 1 (plain text, parsed on the device), 2 (BGZF, inflated there) and 3 (plain
gzip, inflated there): ERR_UNSUPPORTED with one and the same message, which names the read.  A child process per setting:
the driver reads the switches from the environment."""
import gzip
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

_CHILD = r"""
import sys
sys.path.insert(0, %r)
from thermite_amd import capi
data, path, out = sys.argv[1:4]
a = capi.Aligner(capi.Index.from_files(data + "/test_ref.fasta", data + "/test_ref.gtf"), capi.DEFAULT_OPTS)
try:
    capi.align_files(a, [path], out, capi.FMT_BAM)
    print("outcome ok")
except capi.ThermiteError as e:
    print("outcome %%d %%s" %% (e.code, str(e).replace("\n", " ")))
a.close()
"""

TEXT = b"@ok\nACGTACGTACGT\n+\n!!!!!!!!!!!!\n@giant read\n" + b"ACGT" * 17000 + b"\n+\n" + b"!" * 68000 + b"\n"


@pytest.fixture(scope="module")
def outcomes(data_dir, tmp_path_factory):
    import inflate_common as ic
    from thermite_amd import capi
    d = tmp_path_factory.mktemp("failed_read")
    # one file name for every setting: the message may word the path
    files = {None: TEXT, "1": TEXT, "2": ic.members_of(TEXT, 0xff00) + ic.EOF_BLOCK, "3": gzip.compress(TEXT, 6)}
    got = {}
    for switch, body in files.items():
        sub = d / ("fq%s" % switch)
        sub.mkdir()
        path = sub / ("big.fastq" if switch in (None, "1") else "big.fastq.gz")
        path.write_bytes(body)
        env = dict(os.environ)
        env.pop("THM_FASTQ_DEVICE", None)
        env.pop("THM_BAM_SORT", None)
        env["THM_BAM_DEVICE"] = "1"
        if switch is not None:
            env["THM_FASTQ_DEVICE"] = switch
        r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, data_dir, str(path), str(sub / "o.bam")], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("outcome ")]
        assert len(line) == 1, r.stdout
        print("THM_FASTQ_DEVICE=%s: %s" % (switch, line[0]))
        got[switch] = line[0]
    return got, capi.ERR_UNSUPPORTED


@pytest.mark.parametrize("switch", [None, "1", "2", "3"], ids=["unset", "1", "2", "3"])
def test_a_read_the_build_cannot_take_fails_the_run_by_name(outcomes, switch):
    got, code = outcomes
    assert got[switch].startswith("outcome %d " % code) and "giant read" in got[switch], got[switch]
    assert got[switch] == got[None]
