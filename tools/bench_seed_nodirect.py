"""bench.py with the text positions in the k-mer table ignored on every aligner (bit 6 of thm_debug_set_flags: a probe into a
single-suffix bucket reads the suffix array, as with a plain table): the A/B partner of a plain bench.py run; THM_LUT_DIRECT=0
is the other one (the table itself stays plain).  Takes bench.py's arguments and prints its JSON line.
python tools/bench_seed_nodirect.py [bench.py arguments]"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thermite_amd import capi  # noqa: E402

_init = capi.Aligner.__init__


def init(self, *a, **k):
    _init(self, *a, **k)
    self.debug_set_flags(seed_direct=False)


capi.Aligner.__init__ = init
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
