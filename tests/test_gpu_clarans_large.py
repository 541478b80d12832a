"""Device CLARANS for samples beyond 2048 non-medoids / 1024 medoids (lcsgpu_clarans_large[_batch],
clarans_large_chain_kernel) against the reference's CLARANS::operator() -- or, where oracle/_ref is not built, the
host search that the CPU suite pins to it -- on the oracle's float distance triangle.  Every comparison is exact:
the medoid lists are equal.  Families of length 60 keep the CPU oracle's triangle cheap."""
import os
import subprocess
import sys

import numpy as np
import pytest

from famsa_amd import hostlib as host_bind
import oracle_bind
from famsa_amd import seqio

gpu = pytest.mark.gpu
CAP = 32768


@pytest.fixture(scope="module")
def searcher():
    if oracle_bind.have_ref():
        return oracle_bind.Ref().clarans
    return host_bind.Host().clarans


def _family(rng, n, length, mut):
    anc = rng.integers(0, 20, size=length, dtype=np.uint8)
    out = []
    for _ in range(n):
        s = anc.copy()
        m = rng.random(length) < mut
        s[m] = rng.integers(0, 20, size=int(m.sum()), dtype=np.uint8)
        out.append(s[: int(rng.integers(int(length * 0.7), length + 1))].copy())
    return out


def _short(rng, n, lo, hi, alpha):
    return [rng.integers(0, alpha, size=int(rng.integers(lo, hi + 1)), dtype=np.uint8) for _ in range(n)]


def _expected_triangle(oracle, seqs, ids, kind):
    sub = [seqs[i] for i in ids]
    codes, offsets = seqio.pack(sub)
    lcs = oracle.triangle(codes, offsets)
    lens = np.array([len(s) for s in sub], np.uint32)
    return oracle.dist_triangle_f32(lcs, lens, kind)


CASES = [
    # name, generator, n_set, n_sample, k, fixed, fraction, searches, kind
    ("slice-one-over", "family", 2100, 2052, 3, 1, 0.01, 1, 1),        # n - k = 2049: one position in the second slice
    ("slice-edge-4096", "family", 4150, 4104, 8, 1, 0.01, 1, 1),       # n - k = 4096: two full slices
    ("slice-edge-4097", "family", 4150, 4105, 8, 1, 0.01, 1, 1),       # n - k = 4097
    ("old-call-refuses", "family", 2600, 2500, 3, 1, 0.01, 1, 1),
    ("round4-2500-100", "family", 2600, 2500, 100, 1, 0.05, 2, 1),
    ("round4-4300-40", "family", 4400, 4300, 40, 1, 0.01, 2, 1),
    ("slots-beyond-1024", "family", 1500, 1400, 1030, 1, 0.02, 1, 1),  # a second batch of slots, few non-medoids
    ("both-limits", "family", 3500, 3400, 1100, 1, 0.005, 1, 1),
    ("one-medoid", "family", 3100, 3000, 1, 0, 0.02, 2, 1),            # every slot can go negative
    ("ties-short", "short", 2700, 2600, 20, 1, 0.01, 1, 1),
    ("dups-tie-exactly", "dups", 2500, 2400, 12, 1, 0.01, 1, 1),
    ("kind0", "family", 2400, 2300, 25, 1, 0.01, 1, 0),
    ("all-medoids", "family", 1200, 1100, 1100, 1, 0.1, 2, 1),
]


@gpu
@pytest.mark.parametrize("name,gen,n_set,n_sample,k,fixed,frac,iters,kind", CASES, ids=[c[0] for c in CASES])
def test_large_device_clarans_matches_reference(engine, oracle, searcher, name, gen, n_set, n_sample, k, fixed, frac, iters, kind):
    import famsa_amd
    rng = np.random.default_rng(int.from_bytes(name.encode(), "little") % (1 << 31))
    seqs = _family(rng, n_set, 60, 0.25) if gen in ("family", "dups") else _short(rng, n_set, 6, 14, 3)
    if gen == "dups":  # every sequence four times: members at distance 0 of each other, medoids at equal distances
        seqs = [seqs[i // 4] for i in range(n_set)]
    engine.upload_seqs(seqs)
    ids = np.sort(rng.permutation(n_set)[:n_sample]).astype(np.int32)
    tri = _expected_triangle(oracle, seqs, ids, kind)
    want = searcher(tri, n_sample, k, fixed, frac, iters)
    got = engine.clarans_large(ids, k, fixed, frac, iters, kind)
    assert got.tolist() == want.tolist()
    if name == "old-call-refuses":  # lcsgpu_clarans keeps its contract
        with pytest.raises(famsa_amd.LcsGpuError) as e:
            engine.clarans(ids, k, fixed, frac, iters, kind)
        assert "at most" in str(e.value)


@gpu
def test_above_the_cap_is_refused_and_nothing_is_computed(engine):
    import famsa_amd
    rng = np.random.default_rng(11)
    engine.upload_seqs(_short(rng, CAP + 1, 8, 8, 20))
    ids = np.arange(CAP + 1, dtype=np.int32)
    for call in (lambda: engine.clarans_large(ids, 10, 1, 0.01, 1), lambda: engine.clarans_large_batch([ids[:50], ids], [5, 10], 1, 0.01, 1)):
        with pytest.raises(famsa_amd.LcsGpuError) as e:
            call()
        assert "at most" in str(e.value) and "lcsgpu error -6" in str(e.value)  # LCSGPU_E_UNSUPPORTED


@gpu
def test_mixed_batch_equals_every_sample_alone(engine, oracle, searcher):
    """Samples inside and outside the chain kernel's shapes in one lcsgpu_clarans_large_batch: each equals the sample searched
    alone, the in-limit ones equal lcsgpu_clarans_batch, and one large and one small sample equal the reference."""
    rng = np.random.default_rng(314)
    seqs = _family(rng, 2600, 60, 0.25)
    engine.upload_seqs(seqs)
    shapes = [(2000, 100)] * 2 + [(2500, 3)] * 2 + [(310, 7), (1400, 1030), (24, 24)]
    samples = [np.sort(rng.permutation(len(seqs))[:m]).astype(np.int32) for m, _ in shapes]
    ks = [k for _, k in shapes]
    got = engine.clarans_large_batch(samples, ks, 1, 0.02, 2)
    for i, (ids, k) in enumerate(zip(samples, ks)):
        assert got[i].tolist() == engine.clarans_large(ids, k, 1, 0.02, 2).tolist(), i
    small = [0, 1, 4, 6]
    old = engine.clarans_batch([samples[i] for i in small], [ks[i] for i in small], 1, 0.02, 2)
    for j, i in enumerate(small):
        assert got[i].tolist() == old[j].tolist(), i
    for i in (2, 4):
        want = searcher(_expected_triangle(oracle, seqs, samples[i], 1), len(samples[i]), ks[i], 1, 0.02, 2)
        assert got[i].tolist() == want.tolist(), i


@gpu
def test_four_chains_of_one_shape(engine, oracle, searcher):
    """Four 2500 / 3 samples in one call (they share the shape's pre-drawn positions): each equals the sample alone, the first
    the reference.  Under clarans_draws=40 (below) all four run out of positions in the same launches."""
    rng = np.random.default_rng(2718)
    seqs = _family(rng, 2600, 60, 0.25)
    engine.upload_seqs(seqs)
    samples = [np.sort(rng.permutation(len(seqs))[:2500]).astype(np.int32) for _ in range(4)]
    got = engine.clarans_large_batch(samples, 3, 1, 0.01, 1)
    want = searcher(_expected_triangle(oracle, seqs, samples[0], 1), 2500, 3, 1, 0.01, 1)
    assert got[0].tolist() == want.tolist()
    for i in range(1, 4):
        assert got[i].tolist() == engine.clarans_large(samples[i], 3, 1, 0.01, 1).tolist(), i
    assert len({tuple(g.tolist()) for g in got}) > 1  # (different samples: not one answer four times)


def _nested(tune, select):
    assert not os.environ.get("LCSGPU_TUNE"), "the nested runs select no test that starts another"
    env = dict(os.environ)
    env["LCSGPU_TUNE"] = tune  # (read once per process, hence the subprocess)
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k", select],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0 and " passed" in p.stdout, p.stdout[-3000:]


@gpu
def test_where_a_launch_ends_does_not_change_the_large_search():
    """A chain is stopped and started again where it stood: after 40 pre-drawn positions (then twice as many, ...) or 50
    microseconds -- both kernels' slices.  The medoids are the same."""
    _nested("clarans_draws=40,clarans_slice_us=50,clarans_large_slice_us=50",
            "slice-one-over or slots-beyond-1024 or one-medoid or ties-short or dups-tie or kind0 or mixed_batch")


@gpu
def test_same_shape_chains_running_out_of_draws_together():
    """Four chains of one shape that run out of pre-drawn positions at once extend the shape's positions once per round
    (not once per chain: that doubled the array per chain)."""
    _nested("clarans_draws=40", "four_chains_of_one_shape")


def _run_cli(args, env_extra):
    env = dict(os.environ)
    env.update(env_extra)
    env["LCSGPU_PROFILE"] = "1"
    p = subprocess.run(["timeout", "-k", "10", "300", host_bind.CLI, *args], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return p


@gpu
def test_cli_medoidtree_with_a_sample_beyond_the_chain_kernel(tmp_path):
    """famsa-gpu -medoidtree with -sample_size 2600: the sample's search stays on the device (no host notice, the engine's
    CLARANS counted), and the tree is byte for byte the one with the host search and the reference's."""
    rng = np.random.default_rng(1618)
    seqs = _family(rng, 3000, 40, 0.25)  # 30 .. 40 residues (0.7 * 40 = 28 is the generator's floor)
    seqs = [s if len(s) >= 30 else np.concatenate([s, s[: 30 - len(s)]]) for s in seqs]
    codes, offsets = seqio.pack(seqs)
    fasta = str(tmp_path / "in.fasta")
    seqio.to_fasta(codes, offsets, fasta)
    flags = ["-medoidtree", "-gt", "sl", "-gt_export", "-sample_size", "2600", "-cluster_fraction", "0.02", "-cluster_iters", "1",
             "-medoid_threshold", "100", "-subtree_size", "100"]
    dev, hst = str(tmp_path / "dev.dnd"), str(tmp_path / "host.dnd")
    p = _run_cli(flags + [fasta, dev], {})
    assert "searched on the host" not in p.stderr
    calls = [int(ln.split()[1]) for ln in p.stderr.splitlines() if ln.startswith("engine.clarans:")]
    assert calls and calls[0] > 0, p.stderr[-2000:]
    assert "clarans.large:" in p.stderr
    _run_cli(flags + [fasta, hst], {"FAMSA_HOST_TEST": "clarans_host"})
    assert open(dev, "rb").read() == open(hst, "rb").read()
    if oracle_bind.have_ref():
        ref = oracle_bind.Ref()
        h = ref.open_fasta(fasta)
        try:
            want = ref.tree(h, "sl", heuristic=2, subtree=100, sample=2600, threshold=100, cluster_fraction=0.02, cluster_iters=1)
        finally:
            ref.close(h)
        assert open(dev, "rb").read() == want


def test_new_entry_points_reject_a_null_context():
    """CPU: both names are exported and answer LCSGPU_E_INVALID for a NULL context."""
    import ctypes as C
    import famsa_amd
    lib = famsa_amd.load_library()
    ids = (C.c_int32 * 4)(0, 1, 2, 3)
    off = (C.c_int64 * 2)(0, 4)
    k = (C.c_int32 * 1)(2)
    out = (C.c_int32 * 2)()
    assert lib.lcsgpu_clarans_large(None, ids, 4, 1, 2, 1, 0.1, 1, out) == -1
    assert b"NULL" in lib.lcsgpu_last_error()
    assert lib.lcsgpu_clarans_large_batch(None, ids, off, 1, 1, k, 1, 0.1, 1, out) == -1
    assert b"NULL" in lib.lcsgpu_last_error()
