#!/usr/bin/env python3
"""Batch mode against the two ways there were before it, on families of 50 / 200 / 1000 / 4000 members (an ancestor of
60-400 aa, 20 % substitutions per member, lengths cut to 90-100 % of it, as mst_shapes._ragged4 makes them; fixed seed):
512 / 512 / 128 / 16 FASTA files in a temporary directory, -gt sl and -gt upgma, as files per second:
  (a) one famsa-gpu process per file -- the only command-line route before, the baseline;
  (b) a loop over famsa_amd.guide_tree in one process -- the best there was;
  (c) famsa-gpu -batch over the whole directory;
  (c1) the same with FAMSA_HOST_TEST=batch_group_max=1: every file down the one-file route, but on the batch's ONE engine
       context -- what separates the routing (a workgroup per family against lcsgpu_mst_prim's rounds per file) from what
       the shared context and the parallel loading give on their own.  The routing limit is the largest size at which (c)
       is not behind (c1);
  (ch) -gt upgma only: (c) with FAMSA_HOST_TEST=batch_upgma_host -- the chunks' triangles go to the host builders on the worker
       threads, as before lcsgpu_upgma_batch ran a file's merges in a workgroup of its own.
(a) and (b) cost a process start or an engine context per file, so they are timed on the first --files-a / --files-b files
of a size (a rate does not need all 512); (c) takes all of them.  Medians of --reps timed runs after one warm-up.

Before that, the kernel's own part (engine level, one process per setting of LCSGPU_TUNE=mst_batch_square): for one group
of m members, lcsgpu_mst_prim on the group uploaded alone against lcsgpu_mst_prim_batch on it -- wall time of the call and
the kernels' time (for the batch: its launches minus those of lcsgpu_lcs_triangles_batch on the same group = the Prim
launch, with the square's expansion where that is on) -- with the packed triangle read as it is and with the expanded
square.  (One group alone is the kernel's worst case: what it is for is many groups side by side, the `many` column.)
And the same for lcsgpu_upgma_batch: wall time, kernels, the UPGMA launch pair alone (kernels minus those of
lcsgpu_lcs_triangles_batch: the squares with the rows' initial keys, and the merges) and that per merge step.

And for lcsgpu_nj_batch (--nj-kernel-sizes, --skip-nj-kernels), once per thread count (LCSGPU_TUNE nj_group_threads=256 and
=1024, a child each): the NJ launches alone (kernels minus those of lcsgpu_lcs_triangles_batch: the float triangles with the
rows' sums, and the merges), whole and per merge, for one group and for many side by side -- where the two thread counts
cross is NJ_GROUP_WIDE_AT of csrc/fasttree_kernels.h.

--gts (sl, slink, upgma, upgma_modified, nj) / --sizes / --skip-ab / --skip-mst-kernels / --cli narrow a run to some
generators, some family sizes, to the batch legs, and to another build's famsa-gpu.  --parent-cli adds a leg (p): that
build's famsa-gpu -batch (an earlier commit's, on the same machine) timed run by run in alternation with (c), with the
spread (min .. max) of both.

Writes everything to stdout and to --out (default profiles/batch_trees.txt)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

SIZES = (50, 200, 1000, 4000)
COUNTS = (512, 512, 128, 16)
ALPHABET = "ARNDCQEGHILKMFPSTWYV"


def family(rng, members):
    length = int(rng.integers(60, 401))
    anc = rng.integers(0, 20, size=length, dtype=np.uint8)
    out = []
    for _ in range(members):
        s = anc.copy()
        m = rng.random(length) < 0.2
        s[m] = rng.integers(0, 20, size=int(m.sum()), dtype=np.uint8)
        out.append(s[: int(rng.integers(int(length * 0.9), length + 1))])
    return out


def write_fasta(path, seqs):
    letters = np.frombuffer(ALPHABET.encode(), np.uint8)
    with open(path, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">s%d\n" % i + letters[s].tobytes() + b"\n")


def median_of(fn, reps):
    fn()  # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def kernel_child(sizes, reps):
    """Runs in a child per LCSGPU_TUNE setting: one JSON line per group size."""
    import famsa_amd
    rng = np.random.Generator(np.random.PCG64(77))
    eng = famsa_amd.LcsGpu(0)
    for m in sizes:
        seqs = family(rng, m)
        eng.upload_seqs(seqs)
        group = [np.arange(m, dtype=np.int32)]
        rec = {"m": m}
        for name, call in (("mst_prim", lambda: eng.mst_prim(1)), ("batch", lambda: eng.mst_prim_batch(group, 1)),
                           ("triangles", lambda: eng.lcs_triangles_batch(group))):
            call()
            wall, ms = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                call()
                wall.append(time.perf_counter() - t0)
                ms.append(eng.last_kernel_ms()[0])
            rec[name + "_wall_ms"] = 1e3 * statistics.median(wall)
            rec[name + "_kernel_ms"] = statistics.median(ms)
        # many groups of this size side by side: what a chunk looks like to the device
        many = max(1, min(64, 16384 // m))
        groups = [np.arange(m, dtype=np.int32)] * many
        eng.mst_prim_batch(groups, 1)
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            eng.mst_prim_batch(groups, 1)
            wall.append(time.perf_counter() - t0)
        rec["many"] = many
        rec["many_wall_ms"] = 1e3 * statistics.median(wall)
        print(json.dumps(rec), flush=True)
    eng.close()


def upgma_child(sizes, reps):
    """Runs in a child: one JSON line per group size for lcsgpu_upgma_batch."""
    import famsa_amd
    rng = np.random.Generator(np.random.PCG64(77))
    eng = famsa_amd.LcsGpu(0)
    for m in sizes:
        seqs = family(rng, m)
        eng.upload_seqs(seqs)
        group = [np.arange(m, dtype=np.int32)]
        many = max(1, min(64, 16384 // m))
        groups = group * many
        rec = {"m": m, "many": many}
        for name, call in (("upgma", lambda: eng.upgma_batch(group, 1)), ("triangles", lambda: eng.lcs_triangles_batch(group)),
                           ("many", lambda: eng.upgma_batch(groups, 1)), ("many_triangles", lambda: eng.lcs_triangles_batch(groups))):
            res = call()
            if name in ("upgma", "many"):
                assert not res[1].any(), "a family without a tree"
            wall, ms = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                call()
                wall.append(time.perf_counter() - t0)
                ms.append(eng.last_kernel_ms()[0])
            rec[name + "_wall_ms"] = 1e3 * statistics.median(wall)
            rec[name + "_kernel_ms"] = statistics.median(ms)
        print(json.dumps(rec), flush=True)
    eng.close()


def nj_child(sizes, reps):
    """Runs in a child per LCSGPU_TUNE nj_group_threads setting: one JSON line per group size for lcsgpu_nj_batch."""
    import famsa_amd
    rng = np.random.Generator(np.random.PCG64(77))
    eng = famsa_amd.LcsGpu(0)
    for m in sizes:
        seqs = family(rng, m)
        eng.upload_seqs(seqs)
        group = [np.arange(m, dtype=np.int32)]
        many = max(1, min(256, 65536 // m))
        groups = group * many
        rec = {"m": m, "many": many}
        for name, call in (("nj", lambda: eng.nj_batch(group, 1)), ("triangles", lambda: eng.lcs_triangles_batch(group)),
                           ("many", lambda: eng.nj_batch(groups, 1)), ("many_triangles", lambda: eng.lcs_triangles_batch(groups))):
            res = call()
            if name in ("nj", "many"):
                assert not res[1].any(), "a family without a tree"
            wall, ms = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                call()
                wall.append(time.perf_counter() - t0)
                ms.append(eng.last_kernel_ms()[0])
            rec[name + "_wall_ms"] = 1e3 * statistics.median(wall)
            rec[name + "_kernel_ms"] = statistics.median(ms)
        print(json.dumps(rec), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_trees.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--files-a", type=int, default=8)
    ap.add_argument("--files-b", type=int, default=16)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 512 / 512 / 128 / 16 files to make")
    ap.add_argument("--kernel-sizes", default="50,200,256,500,1000,1500,2000,3000,4096")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--upgma-kernel-sizes", default="50,200,256,500,1000,2000,4096")
    ap.add_argument("--nj-kernel-sizes", default="50,200,256,500,1000,2048")
    ap.add_argument("--skip-nj-kernels", action="store_true", help="no lcsgpu_nj_batch kernel table (a build without the call)")
    ap.add_argument("--gts", default="sl,upgma", help="the generators of the files-per-second table (sl, slink, upgma, upgma_modified, nj)")
    ap.add_argument("--sizes", default=",".join(str(m) for m in SIZES), help="the family sizes of the files-per-second table")
    ap.add_argument("--parent-cli", default=None, help="an earlier build's famsa-gpu: leg (p), timed in alternation with (c); with --skip-ab that pair is the whole table")
    ap.add_argument("--skip-ab", action="store_true", help="no (a) / (b) legs: the batch legs only")
    ap.add_argument("--skip-mst-kernels", action="store_true", help="no lcsgpu_mst_prim_batch kernel table")
    ap.add_argument("--skip-upgma-kernels", action="store_true", help="no lcsgpu_upgma_batch kernel table (a build without the call)")
    ap.add_argument("--cli", default=None, help="another build's famsa-gpu for the batch legs")
    ap.add_argument("--kernel-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--upgma-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--nj-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    ksizes = [int(x) for x in args.kernel_sizes.split(",") if x]
    if args.kernel_child:
        kernel_child(ksizes, args.reps)
        return
    if args.upgma_child:
        upgma_child([int(x) for x in args.upgma_kernel_sizes.split(",") if x], args.reps)
        return
    if args.nj_child:
        nj_child([int(x) for x in args.nj_kernel_sizes.split(",") if x], args.reps)
        return

    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:  # (rewritten line by line: a run that is cut short leaves what it had)
            f.write("\n".join(lines) + "\n")

    say("# scripts/batch_trees_bench.py: medians of %d timed runs after one warm-up" % args.reps)
    say()
    say("## one group of m members in one process: lcsgpu_mst_prim (uploaded alone) against lcsgpu_mst_prim_batch")
    say("## wall = the call, kernels = its launches; prim = batch kernels - lcsgpu_lcs_triangles_batch kernels (the Prim launch")
    say("## and, with the square, its expansion); many = that many groups of m in one call, wall per group")
    for square in (() if args.skip_mst_kernels else (0, 1)):
        say("# LCSGPU_TUNE=mst_batch_square=%d (%s)" % (square, "the expanded m x m square" if square else "the packed triangle as it is"))
        say("%6s %14s %14s %14s %14s %12s %16s" % ("m", "mst_prim wall", "mst_prim kern", "batch wall", "batch kern", "prim kern", "many: wall/group"))
        env = dict(os.environ)
        env["LCSGPU_TUNE"] = "mst_batch_square=%d" % square
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-child", "--reps", str(args.reps), "--kernel-sizes",
                            args.kernel_sizes], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        if p.returncode != 0:
            say("FAILED: " + p.stderr[-1500:])
            return 1
        for l in p.stdout.splitlines():
            r = json.loads(l)
            say("%6d %11.3f ms %11.3f ms %11.3f ms %11.3f ms %9.3f ms %10.3f ms x%d" % (
                r["m"], r["mst_prim_wall_ms"], r["mst_prim_kernel_ms"], r["batch_wall_ms"], r["batch_kernel_ms"],
                r["batch_kernel_ms"] - r["triangles_kernel_ms"], r["many_wall_ms"] / r["many"], r["many"]))
        say()
    if not args.skip_upgma_kernels:
        say("## lcsgpu_upgma_batch: one group of m members, and many groups of m in one call (wall and kernels per group);")
        say("## upgma = kernels - lcsgpu_lcs_triangles_batch kernels on the same groups (the squares + the merges); per step = upgma / (m - 1)")
        say("%6s %12s %12s %12s %12s %18s %18s %14s" % ("m", "wall", "kernels", "upgma", "per step", "many: wall/group", "many: upgma/group", "many: per step"))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--upgma-child", "--reps", str(args.reps), "--upgma-kernel-sizes",
                            args.upgma_kernel_sizes], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        if p.returncode != 0:
            say("FAILED: " + p.stderr[-1500:])
            return 1
        for l in p.stdout.splitlines():
            r = json.loads(l)
            one = r["upgma_kernel_ms"] - r["triangles_kernel_ms"]
            many = (r["many_kernel_ms"] - r["many_triangles_kernel_ms"]) / r["many"]
            say("%6d %9.3f ms %9.3f ms %9.3f ms %9.2f us %11.3f ms x%-3d %15.3f ms %11.2f us" % (
                r["m"], r["upgma_wall_ms"], r["upgma_kernel_ms"], one, 1e3 * one / max(r["m"] - 1, 1), r["many_wall_ms"] / r["many"],
                r["many"], many, 1e3 * many / max(r["m"] - 1, 1)))
        say()
    if not args.skip_nj_kernels:
        say("## lcsgpu_nj_batch: one group of m members, and many groups of m in one call; nj = kernels - lcsgpu_lcs_triangles_batch")
        say("## kernels on the same groups (the float triangles with the rows' sums + the merges); per merge = nj / (m - 2);")
        say("## many: nj/group = nj / groups -- throughput with the groups side by side on the compute units, not a group's own time")
        for threads in (256, 1024):
            say("# LCSGPU_TUNE=nj_group_threads=%d" % threads)
            say("%6s %12s %12s %12s %12s %20s %18s" % ("m", "wall", "kernels", "nj", "per merge", "many: wall", "many: nj/group"))
            env = dict(os.environ)
            env["LCSGPU_TUNE"] = "nj_group_threads=%d" % threads
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--nj-child", "--reps", str(args.reps), "--nj-kernel-sizes",
                                args.nj_kernel_sizes], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
            if p.returncode != 0:
                say("FAILED: " + p.stderr[-1500:])
                return 1
            for l in p.stdout.splitlines():
                r = json.loads(l)
                one = r["nj_kernel_ms"] - r["triangles_kernel_ms"]
                many = (r["many_kernel_ms"] - r["many_triangles_kernel_ms"]) / r["many"]
                say("%6d %9.3f ms %9.3f ms %9.3f ms %9.2f us %13.3f ms x%-4d %15.4f ms" % (
                    r["m"], r["nj_wall_ms"], r["nj_kernel_ms"], one, 1e3 * one / max(r["m"] - 2, 1), r["many_wall_ms"], r["many"], many))
            say()
    if args.skip_e2e:
        return 0

    import famsa_amd
    from famsa_amd.hostlib import CLI
    if args.cli:
        CLI = args.cli
    rng = np.random.Generator(np.random.PCG64(2024))
    with tempfile.TemporaryDirectory() as tmp:
        files = {}
        sizes = [int(x) for x in args.sizes.split(",") if x]
        if not sizes or any(m not in SIZES for m in sizes):
            ap.error("--sizes takes some of %s" % ",".join(str(m) for m in SIZES))
        for m, count in zip(SIZES, COUNTS):
            if m not in sizes:
                continue
            count = max(1, int(round(count * args.scale)))
            files[m] = []
            for k in range(count):
                path = os.path.join(tmp, "f%d_%04d.fasta" % (m, k))
                write_fasta(path, family(rng, m))
                files[m].append(path)
        out_dir = os.path.join(tmp, "out")
        os.makedirs(out_dir)

        def outs(paths):
            return [os.path.join(out_dir, os.path.basename(p) + ".dnd") for p in paths]

        say("## files per second; (a) one famsa-gpu process per file (first %d files), (b) famsa_amd.guide_tree in a loop in one" % args.files_a)
        say("## process (first %d files), (c) famsa-gpu -batch (all files of the size)" % args.files_b)
        say("## (c1) = (c) with every file sent down the one-file route on the batch's one engine context; (c4096) = (c) with the routing")
        say("## limit at the kernel's cap: the chunks take every size; (ch) = (c) with the UPGMA / NJ merges in the host builders")
        if args.parent_cli:
            say("## (p) = %s -batch, run by run in alternation with (c): medians, and [min .. max] of the timed runs" % args.parent_cli)
        say("%6s %6s %8s %12s %12s %12s %12s %14s %12s %8s %8s" % ("gt", "m", "files", "(a) files/s", "(b) files/s", "(c) files/s", "(c1) files/s",
                                                               "(c4096) files/s", "(ch) files/s", "c / a", "c / b"))
        nan = float("nan")
        for gt in [g for g in args.gts.split(",") if g]:
            for m in sizes:
                fa, fb, fc = files[m][: args.files_a], files[m][: args.files_b], files[m]

                def run_a():
                    for src, dst in zip(fa, outs(fa)):
                        subprocess.run([CLI, "-gt", gt, "-gt_export", src, dst], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)

                def run_b():
                    for src in fb:
                        famsa_amd.guide_tree(src, gt=gt)

                lst = os.path.join(tmp, "list_%d.txt" % m)
                with open(lst, "w") as f:
                    for src, dst in zip(fc, outs(fc)):
                        f.write("%s\t%s\n" % (src, dst))

                def run_c(hook=None, cli=None):
                    env = dict(os.environ)
                    env.pop("FAMSA_HOST_TEST", None)
                    if hook:
                        env["FAMSA_HOST_TEST"] = hook
                    subprocess.run([cli or CLI, "-gt", gt, "-gt_export", "-batch", lst], check=True, stdout=subprocess.DEVNULL,
                                   stderr=subprocess.DEVNULL, env=env)

                a = nan if args.skip_ab else len(fa) / median_of(run_a, args.reps)
                b = nan if args.skip_ab else len(fb) / median_of(run_b, args.reps)
                if args.parent_cli:  # this build and the earlier one, run by run in turn, after a warm-up of each
                    run_c()
                    run_c(cli=args.parent_cli)
                    tc, tp = [], []
                    for _ in range(args.reps):
                        for cli, times in ((None, tc), (args.parent_cli, tp)):
                            t0 = time.perf_counter()
                            run_c(cli=cli)
                            times.append(time.perf_counter() - t0)
                    say("%6s %6d %8d (c) %.1f files/s [%.1f .. %.1f]   (p) %.1f files/s [%.1f .. %.1f]   c / p %.2f" % (
                        gt, m, len(fc), len(fc) / statistics.median(tc), len(fc) / max(tc), len(fc) / min(tc),
                        len(fc) / statistics.median(tp), len(fc) / max(tp), len(fc) / min(tp), statistics.median(tp) / statistics.median(tc)))
                    parent_out = [open(p, "rb").read() for p in outs(fc)]  # (the earlier build ran last)
                    run_c()
                    assert parent_out == [open(p, "rb").read() for p in outs(fc)], (gt, m, "this build's bytes differ from the earlier build's")
                    if args.skip_ab:
                        continue
                c = len(fc) / median_of(run_c, args.reps)
                c1 = len(fc) / median_of(lambda: run_c("batch_group_max=1"), args.reps)
                c4096 = len(fc) / median_of(lambda: run_c("batch_group_max=4096"), args.reps)
                ch = len(fc) / median_of(lambda: run_c("batch_upgma_host"), args.reps) if gt.startswith("upgma") else \
                    len(fc) / median_of(lambda: run_c("batch_nj_host"), args.reps) if gt == "nj" else nan
                say("%6s %6d %8d %12.1f %12.1f %12.1f %12.1f %14.1f %12.1f %8.1f %8.1f" % (gt, m, len(fc), a, b, c, c1, c4096, ch, c / a, c / b))
                # the batch's outputs are the one-file command's (spot check on the files (a) wrote last)
                run_a()
                one = [open(p, "rb").read() for p in outs(fa)]
                run_c()
                assert one == [open(p, "rb").read() for p in outs(fa)], (gt, m)
        last_gt = [g for g in args.gts.split(",") if g][-1]
        p = subprocess.run([CLI, "-gt", last_gt, "-gt_export", "-batch", lst, "-v"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        say()
        say("## famsa-gpu -gt %s -gt_export -batch -v on the m = %d list" % (last_gt, sizes[-1]))
        for l in p.stderr.splitlines():
            say(l)
    return 0


if __name__ == "__main__":
    sys.exit(main())
