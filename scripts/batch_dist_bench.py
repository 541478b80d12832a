#!/usr/bin/env python3
"""Batch mode for distance matrices against the two ways there were before it, on the family sets of
scripts/batch_trees_bench.py (50 / 200 / 1000 members x 512 / 512 / 128 FASTA files in a temporary directory; fixed seed),
lower form, default distance, as files per second:
  (a) one famsa-gpu -dist_export process per file;
  (b) a loop over famsa_amd.dist_export in one process;
  (c) famsa-gpu -dist_export -batch over the whole directory.
(a) and (b) cost a process start or the per-file text slots, so they are timed on the first --files-a / --files-b files of a
size; (c) takes all of them.  The routes are run in turn, --reps times each after one warm-up of each (a run here is mostly
process start and file writes, and the spread from run to run is large): medians, and [min .. max] of the timed runs.
--hooks adds legs of (c) under a FAMSA_HOST_TEST setting each (e.g. batch_values=1073741824: one chunk for everything, so
that no file is written before the last one is computed).  Then the batch's own split of its time (-v) per size.

Writes everything to stdout and to --out (default profiles/batch_dist.txt)."""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
from batch_trees_bench import family, write_fasta  # noqa: E402

SIZES = (50, 200, 1000)
COUNTS = (512, 512, 128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_dist.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--files-a", type=int, default=8)
    ap.add_argument("--files-b", type=int, default=16)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 512 / 512 / 128 files to make")
    ap.add_argument("--sizes", default=",".join(str(m) for m in SIZES))
    ap.add_argument("--hooks", default="", help="FAMSA_HOST_TEST settings for further legs of (c), separated by ';'")
    ap.add_argument("--square", action="store_true", help="-square_matrix instead of the lower form")
    args = ap.parse_args()
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:  # (rewritten line by line: a run that is cut short leaves what it had)
            f.write("\n".join(lines) + "\n")

    import famsa_amd
    from famsa_amd.hostlib import CLI
    mode = ["-square_matrix"] if args.square else []
    hooks = [h for h in args.hooks.split(";") if h]
    rng = np.random.Generator(np.random.PCG64(2024))
    sizes = [int(x) for x in args.sizes.split(",") if x]
    say("# scripts/batch_dist_bench.py: -dist_export%s, %d timed runs per route after one warm-up, the routes in turn" % (" -square_matrix" if args.square else "", args.reps))
    say("# files per second: median [slowest .. fastest run]")
    say("# (a) one famsa-gpu process per file (first %d files), (b) famsa_amd.dist_export in a loop (first %d files), (c) famsa-gpu -batch (all)" % (
        args.files_a, args.files_b))
    with tempfile.TemporaryDirectory() as tmp:
        out_dir = os.path.join(tmp, "out")
        os.makedirs(out_dir)
        verbose = {}
        for m, count in zip(SIZES, COUNTS):
            if m not in sizes:
                continue
            count = max(1, int(round(count * args.scale)))
            files = []
            for k in range(count):
                path = os.path.join(tmp, "f%d_%04d.fasta" % (m, k))
                write_fasta(path, family(rng, m))
                files.append(path)

            def outs(paths):
                return [os.path.join(out_dir, os.path.basename(p) + ".csv") for p in paths]

            fa, fb = files[: args.files_a], files[: args.files_b]
            lst = os.path.join(tmp, "list_%d.txt" % m)
            with open(lst, "w") as f:
                for src, dst in zip(files, outs(files)):
                    f.write("%s\t%s\n" % (src, dst))

            def run_a():
                for src, dst in zip(fa, outs(fa)):
                    subprocess.run([CLI, "-dist_export", *mode, src, dst], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

            def run_b():
                for src, dst in zip(fb, outs(fb)):
                    famsa_amd.dist_export(src, dst, square_matrix=args.square)

            def run_c(hook=None, keep=None):
                env = dict(os.environ)
                env.pop("FAMSA_HOST_TEST", None)
                if hook:
                    env["FAMSA_HOST_TEST"] = hook
                p = subprocess.run([CLI, "-dist_export", *mode, "-batch", lst, "-v"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                                   text=True, env=env)
                if keep is not None:
                    keep.append(p.stderr)

            legs = [("(a)", run_a, len(fa)), ("(b)", run_b, len(fb)), ("(c)", run_c, len(files))]
            legs += [("(c) " + h, (lambda h=h: run_c(h)), len(files)) for h in hooks]
            # what (a) writes is what (c) writes
            run_a()
            one = [open(p, "rb").read() for p in outs(fa)]
            for _, fn, _ in legs[1:]:
                fn()  # warm-up; (c) ran last
            assert one == [open(p, "rb").read() for p in outs(fa)], (m, "the batch's bytes differ from the one-file command's")
            times = {name: [] for name, _, _ in legs}
            for _ in range(args.reps):
                for name, fn, _ in legs:
                    t0 = time.perf_counter()
                    fn()
                    times[name].append(time.perf_counter() - t0)
            text_mb = sum(os.path.getsize(p) for p in outs(files)) / 1e6
            say()
            say("## m = %d: %d files, %.1f MB of text (%.2f MB per file)" % (m, len(files), text_mb, text_mb / len(files)))
            med = {}
            for name, _, k in legs:
                t = times[name]
                med[name] = k / statistics.median(t)
                say("%-28s %9.1f files/s [%.1f .. %.1f]" % (name, med[name], k / max(t), k / min(t)))
            say("%-28s %9.1f    c / b %.1f" % ("c / a", med["(c)"] / med["(a)"], med["(c)"] / med["(b)"]))
            keep = []
            run_c(keep=keep)
            verbose[m] = keep[0]
            for p in outs(files):
                os.remove(p)
            for p in files:
                os.remove(p)
        for m, text in verbose.items():
            say()
            say("## famsa-gpu -dist_export -batch -v on the m = %d list" % m)
            for l in text.splitlines():
                say(l)
    return 0


if __name__ == "__main__":
    sys.exit(main())
