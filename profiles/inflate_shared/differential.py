"""One-off differential run for the shared DEFLATE block decoder (DESIGN.md sections 4.13 and 4.14): the model programs
of two trees -- tests/cpp/inflate_model_main.cpp and tests/cpp/gzip_model_main.cpp, built from the parent commit and from
this one -- over the same inputs, every output file compared byte for byte (for gzip the .log and .states files too).

  python profiles/inflate_shared/differential.py WORK OLD_INFLATE NEW_INFLATE OLD_GZIP NEW_GZIP [ASAN_INFLATE ASAN_GZIP]

Inputs: every fixture of tests/inflate_common.py at head lengths 0, 1, 3, 17; every fixture of tests/gzip_common.py at
every MODEL_CHUNKS x MODEL_SLICES and the last=0 cut case; 3 000 single-bit mutants of four BGZF members (head length 3)
and 1 000 of one gzip member (chunks of 64 and 4096 bytes, whole), random.Random(1), every second flip in the first 100
payload bytes.  With the two sanitizer builds (stand-alone programs, nothing preloaded) the corpus goes through them as
well and their outputs are compared with the new models'.  Prints the histograms of the old models' verdicts over the
two corpora and the count of differing files; exit status 1 when a file differs or a condition on the corpus fails."""
import collections
import filecmp
import os
import random
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import gzip_common as gc       # noqa: E402
import inflate_common as ic    # noqa: E402

BATCH = 400


def flips(rng, data, lo, hi, n):
    out = []
    for i in range(n):
        byte = rng.randrange(lo, min(lo + 100, hi)) if i % 2 else rng.randrange(lo, hi)
        bad = bytearray(data)
        bad[byte] ^= 1 << rng.randrange(8)
        out.append(bytes(bad))
    return out


def bgzf_corpus():
    rng, out = random.Random(1), []
    for name in ("fixed_3000_fastq", "dynamic_fastq_level_6", "fibonacci_code_length_15", "stored_two_blocks"):
        m = ic.well_formed()[name].members
        if m.endswith(ic.EOF_BLOCK) and len(m) > len(ic.EOF_BLOCK):
            m = m[: -len(ic.EOF_BLOCK)]
        out += [("%s_%03d" % (name, k), b) for k, b in enumerate(flips(rng, m, 18, len(m) - 8, 750))]
    return out


def gzip_corpus():
    m = gc.member(gc.text()[:60000])
    return [("mutant_%04d" % k, b) for k, b in enumerate(flips(random.Random(1), m, 10, len(m) - 8, 1000))]


def run(exe, lead, inputs, src, dst, tag, env=None):
    """the inputs (written once under src) through exe in batches; outputs dst/<name>.<tag>.out*"""
    os.makedirs(src, exist_ok=True)
    os.makedirs(dst, exist_ok=True)
    for name, data in inputs:
        p = os.path.join(src, name + ".in")
        if not os.path.exists(p):
            open(p, "wb").write(data)
    for at in range(0, len(inputs), BATCH):
        args = []
        for name, _ in inputs[at: at + BATCH]:
            args += [os.path.join(src, name + ".in"), os.path.join(dst, "%s.%s.out" % (name, tag))]
        r = subprocess.run([exe] + [str(x) for x in lead] + args, capture_output=True, env=env)
        if r.returncode != 0 or r.stderr:
            sys.exit("%s %s: exit %d\n%s" % (exe, lead, r.returncode, r.stderr.decode(errors="replace")[-4000:]))


def differing(a, b):
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    bad = [n for n in names if not (os.path.exists(os.path.join(a, n)) and os.path.exists(os.path.join(b, n)) and
                                    filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False))]
    return len(names), bad


def bgzf_verdict(path):
    w = open(path, "rb").readline().split()
    return "ok" if w[0] == b"ok" else "walk" if w[0] == b"walk" else int(w[2])


def gzip_verdict(path):
    status = int(open(path + ".log").read().splitlines()[-1].split()[1])
    return status or "ok"


def main():
    work, old_inf, new_inf, old_gz, new_gz = sys.argv[1:6]
    asan = sys.argv[6:8]
    src = os.path.join(work, "in")
    fail = False
    bgzf_fix = [(k, v[0]) for k, v in ic.corrupt().items()] + [(k, v.members) for k, v in ic.not_for_device().items()] + \
               [(k, v.members) for k, v in ic.well_formed().items()]
    gzip_fix = [(k, v[0]) for k, v in gc.corrupt().items()] + [(k, v[0].stream) for k, v in gc.declined().items()] + \
               [(k, v.stream) for k, v in gc.well_formed().items()]
    cut = [("cut", gc.well_formed()["level6"].stream[:100001])]
    bc, gzc = bgzf_corpus(), gzip_corpus()
    for which, exe_i, exe_g in (("old", old_inf, old_gz), ("new", new_inf, new_gz)) + ((("asan",) + tuple(asan),) if asan else ()):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1") if which == "asan" else None
        if env:
            env.pop("LD_PRELOAD", None)
        if which != "asan":
            for h in (0, 1, 3, 17):
                run(exe_i, [h], bgzf_fix, src + "_bgzf_fix", os.path.join(work, which, "bgzf_fix"), "h%d" % h)
            for chunk in gc.MODEL_CHUNKS:
                for sl in gc.MODEL_SLICES:
                    run(exe_g, [chunk, sl, 1], gzip_fix, src + "_gzip_fix", os.path.join(work, which, "gzip_fix"), "%d_%d_1" % (chunk, sl))
            run(exe_g, [4096, 0, 0], cut, src + "_gzip_fix", os.path.join(work, which, "gzip_fix"), "4096_0_0")
        run(exe_i, [3], bc, src + "_bgzf_corpus", os.path.join(work, which, "bgzf_corpus"), "h3", env)
        for chunk in (64, 4096):
            run(exe_g, [chunk, 0, 1], gzc, src + "_gzip_corpus", os.path.join(work, which, "gzip_corpus"), "%d_0_1" % chunk, env)
    # the old models' verdicts over the corpora, and the conditions on them
    hb = collections.Counter(bgzf_verdict(os.path.join(work, "old", "bgzf_corpus", n + ".h3.out")) for n, _ in bc)
    print("BGZF corpus, %d mutants, old model's verdicts: %s" % (len(bc), sorted(hb.items(), key=str)))
    fail |= not all(hb[s] for s in (3, 4, 5, 6, 7, 8, 10)) or hb["ok"] > len(bc) // 100
    for chunk in (64, 4096):
        hg = collections.Counter(gzip_verdict(os.path.join(work, "old", "gzip_corpus", "%s.%d_0_1.out" % (n, chunk))) for n, _ in gzc)
        print("gzip corpus, %d mutants, chunk %d, old model's verdicts: %s" % (len(gzc), chunk, sorted(hg.items(), key=str)))
        fail |= not all(hg[s] for s in (4, 5, 6, 8)) or hg["ok"] > len(gzc) // 100
    if fail:
        print("a condition on the corpus does not hold")
    for part in ("bgzf_fix", "gzip_fix", "bgzf_corpus", "gzip_corpus"):
        n, bad = differing(os.path.join(work, "old", part), os.path.join(work, "new", part))
        print("old against new, %s: %d files compared, %d differ %s" % (part, n, len(bad), bad[:10]))
        fail |= bool(bad) or n == 0
    if asan:
        for part in ("bgzf_corpus", "gzip_corpus"):
            n, bad = differing(os.path.join(work, "new", part), os.path.join(work, "asan", part))
            print("new against its ASan + UBSan build, %s: %d files compared, %d differ %s; no sanitizer report" % (part, n, len(bad), bad[:10]))
            fail |= bool(bad) or n == 0
    sys.exit(1 if fail else 0)


if __name__ == "__main__":
    main()
