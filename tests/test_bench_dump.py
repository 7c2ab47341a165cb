"""bench.py --dump-outputs without a GPU: dump_outputs on the oracle's result of a chrM batch (the same canonical layout
the HIP path returns) writes a fixed sample of the reads with exactly their alignment records and op bytes."""
import os
import types

import numpy as np

import bench
from oracle import pyoracle as orc
from thermite_amd import capi, refdata, synth


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_sample_is_the_batch_result(data_dir, tmp_path, monkeypatch):
    t = refdata.load_reference(os.path.join(data_dir, "GRCh38-2020-A-chrM.fasta"), os.path.join(data_dir, "GRCh38-2020-A-chrM.gtf"))
    bases, off, _ = synth.simulate_reads(t, 3000, 91)
    r = orc.Index(t, sa=capi.build_suffix_array(t["text"])).align_batch(bases, off, capi.CI_OPTS, n_threads=4)
    g = types.SimpleNamespace(n_reads=r.n, offsets=r.offsets, alns=r.alns, ops=r.ops, status=None)
    monkeypatch.setattr(bench, "DUMP_READS", 700)
    bench.dump_outputs(str(tmp_path / "a"), g)
    bench.dump_outputs(str(tmp_path / "b"), g)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)  # the sample is fixed
    names = [f for f in capi.ALN_DT.names if f != "pad_"]
    assert set(a) == {"reads", "aln_count", "read_status", "ops"} | {"aln_" + f for f in names}
    assert all(v.dtype == (np.float32 if k == "ops" else np.float64) for k, v in a.items())

    reads = a["reads"].astype(np.int64)
    assert len(reads) == 700 and np.all(np.diff(reads) > 0) and reads[-1] < 3000
    o = r.offsets.astype(np.int64)
    assert np.array_equal(a["aln_count"], o[reads + 1] - o[reads]) and not a["read_status"].any()
    rows = np.concatenate([np.arange(o[i], o[i + 1]) for i in reads])
    assert len(rows) > 600
    for f in names:
        assert np.array_equal(a["aln_" + f], r.alns[f][rows].astype(np.float64)), f
    ops = [r.ops[s: s + n] for x in r.alns[rows] for s, n in ((x["ops_off"], x["ops_len"]), (x["tx_ops_off"], x["tx_ops_len"]))]
    assert np.array_equal(a["ops"], np.concatenate(ops).astype(np.float32))
    assert sum(v.nbytes for v in a.values()) < 64 << 20
