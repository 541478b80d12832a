#!/usr/bin/env python3
"""One timed CLARANS search of a sample beyond the chain kernel's shapes -- dev tool behind profiles/clarans_large.txt.

    clarans_large_bench.py MEMBERS MEDOIDS device|host [FRACTION [SEARCHES]]

device: lcsgpu_clarans_large, the whole call (sample triangle, float matrix, chains) after a small warm-up call.
host:   the one-thread host search (what such a sample got before) on the same sample's float triangle -- the LCS
        triangle from the engine, the float transform from the oracle; the search alone is timed.
One run per process; prints one line with the milliseconds and the first medoids (both legs must print the same)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import famsa_amd
from famsa_amd import hostlib

n, k, what = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
frac = float(sys.argv[4]) if len(sys.argv) > 4 else 0.1
searches = int(sys.argv[5]) if len(sys.argv) > 5 else 2
rng = np.random.default_rng(n)
L = 60
anc = rng.integers(0, 20, size=L, dtype=np.uint8)
seqs = []
for _ in range(n + 100):
    s = anc.copy()
    m = rng.random(L) < 0.25
    s[m] = rng.integers(0, 20, size=int(m.sum()), dtype=np.uint8)
    seqs.append(s[: int(rng.integers(int(L * 0.7), L + 1))].copy())
ids = np.sort(rng.permutation(n + 100)[:n]).astype(np.int32)
eng = famsa_amd.LcsGpu(0)
eng.upload_seqs(seqs)
if what == "device":
    eng.clarans_large(ids[:2100], 3, 1, 0.01, 1)  # warm-up: the code objects, the first work area
    t0 = time.time()
    med = eng.clarans_large(ids, k, 1, frac, searches)
    ms = 1e3 * (time.time() - t0)
else:
    import oracle_bind
    lcs = eng.lcs_triangle_ids(ids, dtype=np.uint32)
    tri = oracle_bind.Oracle().dist_triangle_f32(lcs, np.array([len(seqs[i]) for i in ids], np.uint32), 1)
    t0 = time.time()
    med = hostlib.Host().clarans(tri, n, k, 1, frac, searches)
    ms = 1e3 * (time.time() - t0)
print("clarans %d/%d fraction %g x%d %s: %.1f ms  medoids[:6]=%s" % (n, k, frac, searches, what, ms, med[:6].tolist()), flush=True)
