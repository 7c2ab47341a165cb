"""What the extend stage pays per read of the finisher's classes: batches of reads of ONE class -- whole-read exact matches
(class E), one substitution between two SMEMs (class S), drawn from the benchmark's reference inside single exons -- and a
batch drawn as bench.py draws it, each run with the finisher off and on (thm_debug_set_flags bits 12..15; a library without
the finisher ignores the bits and gives the "off" figure twice).  Prints one JSON line per batch with the stage times.
python tools/smem_class_cost.py [--reads 500000] [--ref-len N] [--steps 12]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thermite_amd import capi, refdata, synth  # noqa: E402

_ACGT = np.frombuffer(b"ACGT", np.uint8)


def class_reads(t, n, L, rng, subst):
    """n reads inside single exons of the forward copy (half of them reverse-complemented); subst: one substitution at a
    position with both flanks of 20 bases and more"""
    r0 = t["refs"][0]
    e = t["exons"]
    on = (e["start"] >= r0["start_idx"]) & (e["end"] <= r0["end_idx"]) & (e["end"] - e["start"] >= L)
    ex = np.unique(np.stack([e["start"][on], e["end"][on]], axis=1).astype(np.int64), axis=0)
    k = rng.integers(0, len(ex), n)
    s = ex[k, 0] + (rng.random(n) * (ex[k, 1] - ex[k, 0] - L + 1)).astype(np.int64) - int(r0["start_idx"])
    reads = t["text"][s[:, None] + np.arange(L, dtype=np.int64)[None, :]].copy()
    if subst:
        p = rng.integers(20, L - 20, n)
        code = np.full(256, 0, np.uint8)
        code[_ACGT] = np.arange(4, dtype=np.uint8)
        old = code[reads[np.arange(n), p]]
        reads[np.arange(n), p] = _ACGT[(old + rng.integers(1, 4, n).astype(np.uint8)) % 4]
    flip = rng.random(n) < 0.5
    reads[flip] = refdata._COMP[reads[flip][:, ::-1]]
    return np.ascontiguousarray(reads.reshape(-1)), (np.arange(n + 1, dtype=np.uint64) * np.uint64(L)).astype("<u8")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=500000)
    ap.add_argument("--ref-len", type=int, default=synth.CHR21_LEN)
    ap.add_argument("--read-len", type=int, default=91)
    ap.add_argument("--steps", type=int, default=12)
    args = ap.parse_args()
    t = synth.synth_reference(length=args.ref_len)
    ix = capi.Index(t)
    rng = np.random.default_rng(1)
    L, n = args.read_len, args.reads
    batches = {
        "class_E": class_reads(t, n, L, rng, False),
        "class_S": class_reads(t, n, L, rng, True),
        "bench": synth.simulate_reads(t, n, L, sub_rate=0.01, indel_rate=0.001, stream=100)[:2],
    }
    for name, (bases, off) in batches.items():
        for on in (False, True):
            a = capi.Aligner(ix, capi.CI_OPTS)
            a.debug_set_flags(finish_exact=on, finish_subst=on)
            a.upload(bases, off)
            for _ in range(3):
                a.run()
                a.sync()
            tm = {k: [] for k in capi.TIMING_NAMES}
            for _ in range(args.steps):
                a.run()
                a.sync()
                for k, v in a.timings().items():
                    tm[k].append(v)
            stats = a.debug_smem_finish_stats() if hasattr(capi.lib(), "thm_debug_smem_finish_stats") else None
            print(json.dumps({"batch": name, "reads": n, "finisher": on, "finish_stats": stats,
                              "median_ms": {k: round(float(np.median(v)), 4) for k, v in tm.items() if k in ("seed", "plan", "extend", "compact", "total")},
                              "min_extend_ms": round(float(np.min(tm["extend"])), 4), "max_extend_ms": round(float(np.max(tm["extend"])), 4)}), flush=True)
            a.close()
    ix.close()


if __name__ == "__main__":
    main()
