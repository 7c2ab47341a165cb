"""bench.py with classes of the finisher (thermite_amd/csrc/kernels_finish.hip) switched off on every aligner (bits 12 and 14
of thm_debug_set_flags): the A/B partner of a plain bench.py run.  THM_FINISH names what stays ON: "" (default: nothing, every
read takes the extend kernel, as before the finisher), "E" (whole-read exact matches only), "S" (one substitution between two
SMEMs only) or "ES".  Takes bench.py's arguments and prints its JSON line, then one line with the finisher's counts of the last
batch.
THM_FINISH=E python tools/bench_smem_finish.py [bench.py arguments]"""
import atexit
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thermite_amd import capi  # noqa: E402

ON = os.environ.get("THM_FINISH", "").upper()
_init = capi.Aligner.__init__
_close = capi.Aligner.close
_last = {}


def init(self, *a, **k):
    _init(self, *a, **k)
    self.debug_set_flags(finish_exact="E" in ON, finish_subst="S" in ON)


def close(self):
    if getattr(self, "h", None):
        try:
            _last["stats"] = self.debug_smem_finish_stats()
        except Exception:
            pass
    _close(self)


capi.Aligner.__init__ = init
capi.Aligner.close = close
atexit.register(lambda: print("[bench_smem_finish] classes on: %r; last batch (E finished, E left, S finished, S left): %s" % (ON, _last.get("stats")),
                              file=sys.stderr))
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
