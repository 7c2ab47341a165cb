"""bench.py with the seed stage's cell rule off on every aligner (bit 16 of thm_debug_set_flags: a grid cell whose two grid points
do not share a stored end has all its inner positions probed, thermite_amd/csrc/seed_bounds.h): the A/B partner of a plain
bench.py run.  Takes bench.py's arguments and prints its JSON line.   python tools/bench_seed_nobounds.py [bench.py arguments]"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thermite_amd import capi  # noqa: E402

_init = capi.Aligner.__init__


def init(self, *a, **k):
    _init(self, *a, **k)
    self.debug_set_flags(seed_bounds=False)


capi.Aligner.__init__ = init
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
