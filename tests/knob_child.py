"""One device run of a workload of knob_common.py in a fresh process: the run-time knobs of INTEGRATION.md section 6 are
read once per process, so tests/test_gpu_knobs.py starts this script with the knob in its environment.

    python knob_child.py WORKLOAD WIDTH OUT.npz [--tpr 0|1] [--rounds R]

WIDTH is 32 or 64 (coordinate width of the index).  Writes every run's offsets, records, op bytes, statuses, counters and
problem-parallel stats, the thm_smems_batch output where the workload asks for it, and the thm_debug_knobs report.  No
oracle work and no comparison happens here."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import knob_common  # noqa: E402
from thermite_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload")
    ap.add_argument("width", type=int, choices=(32, 64))
    ap.add_argument("out")
    ap.add_argument("--tpr", type=int, choices=(0, 1), default=None)
    ap.add_argument("--rounds", type=int, default=0)
    args = ap.parse_args()
    n_cu = knob_common.device_n_cu() if args.workload == "compact" else knob_common.N_CU_DEFAULT
    w = knob_common.build(args.workload, n_cu)
    ix = capi.Index(w["tables"], wide=args.width == 64)
    out = knob_common.run_workload(w, ix, tpr=None if args.tpr is None else bool(args.tpr), rounds=args.rounds)
    ix.close()
    np.savez(args.out, **out)


if __name__ == "__main__":
    main()
