"""One device run of the reads of seed_direct_common.py in a fresh process: THM_LUT_DIRECT is read when the device copy
of an index is made, so tests/test_gpu_seed_direct.py starts this script with the knob in its environment.

    python seed_direct_child.py WIDTH OUT.npz

WIDTH is 32 or 64.  Saves what seed_direct_common.device_run returns; no oracle work and no comparison happens here."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import seed_direct_common as sd  # noqa: E402


def main():
    wide = sys.argv[1] == "64"
    ix = sd.make_index(sd.tables(), wide)
    bases, off = sd.case_batch("all")
    out = sd.device_run(ix, bases, off)
    ix.close()
    np.savez(sys.argv[2], **out)


if __name__ == "__main__":
    main()
