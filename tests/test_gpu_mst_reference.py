"""Every way lcsgpu_mst_prim reaches a tree -- the streaming passes over a resident triangle, the launch with round 0
fused in, the rounds that recompute every LCS value, the hybrid of resident and recomputed rows, the step-by-step Prim
kernel -- and the row-block shard protocol and the group call above them, against a reference that is NOT the engine:
MSTPrim's recurrence in plain Python (mst_ref.prim_edges) over the oracle's LCS values and scalar distances, on the
degenerate sets of mst_shapes.py: whole column blocks of empty sequences, LCS-0 pairs, exact duplicates, ties the ids
settle, sizes around the 256-column tile, the longest sequence a 16-bit record holds.

What these sets found: with a whole aligned 256-id block of empty sequences (zero_first, zero_last, zero_only) the
rounds that recompute let every tile of that column block go -- fuse_tile_is_useless took "the longest column with a
pair is 0 long" for "no column has a pair" -- so the block's vertices lost their (huge-distance, id-decided) edges:
another tree than the passes give (zero_last: vertex 554 took (255, 554) instead of (554, 555)), or the clean error "a
Boruvka round added no edge" (zero_first, zero_only)."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import famsa_amd
import mst_ref
import mst_shapes
from famsa_amd import seqio
from famsa_amd.hostlib import CLI
from famsa_amd.lcsgpu import MST_COMPUTE, MST_TRIANGLE_ORIENTATION
from famsa_amd.rowblock import row_cuts, pairs_in_rows, sharded_mst_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
MODES = (None, "passes", "fused", "recompute", "prim")
KINDS = (1, 0, 1 | MST_TRIANGLE_ORIENTATION)
SHARD_SHAPES = ["zero_last", "allx", "ties", "ragged4_sorted", "ragged4_shuffled"]  # b, e, g, j
_REF = {}


def _same(a, b):
    return (a["from"] == b["from"]).all() and (a["to"] == b["to"]).all() and \
        (a["dist"].view(np.uint64) == b["dist"].view(np.uint64)).all()


def _first_difference(got, want):
    for k in range(len(want)):
        if tuple(got[k]) != tuple(want[k]) or got["dist"][k:k + 1].view(np.uint64) != want["dist"][k:k + 1].view(np.uint64):
            return "edge %d: got %s, want %s" % (k, got[k], want[k])
    return "no difference"


def _reference(oracle, name):
    """(sequences, {kind: (D, edges)}) of a named set: the scalar reference, computed once and shared read-only."""
    if name not in _REF:
        seqs = mst_shapes.build(name)
        codes, offsets = seqio.pack(seqs)
        by_kind = {}
        for kind in (1, 0):
            D = mst_ref.pair_distances(oracle, codes, offsets, kind)
            want = mst_ref.prim_edges(D)
            D.flags.writeable = False
            want.flags.writeable = False
            by_kind[kind] = (D, want)
        _REF[name] = (seqs, by_kind)
    return _REF[name]


def _set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("LCSGPU_MST_MODE", raising=False)
    else:
        monkeypatch.setenv("LCSGPU_MST_MODE", mode)


@pytest.mark.parametrize("name", mst_shapes.GPU_SHAPES)
def test_every_mode_against_prim_over_the_oracle(engine, oracle, monkeypatch, name):
    """One set, kinds 1, 0 and 1 | TRIANGLE_ORIENTATION (no member is orientation sensitive: the flag must change
    nothing), LCSGPU_MST_MODE unset / passes / fused / recompute / prim: from, to, the distance's bits and the order.
    (maxlen: the oracle's row of the 65535-residue member takes a tenth of a second on the CPU, so the whole reference
    is the oracle's.  On the GPU the one pair 65535 x 65534 is a single lane's walk of about 2 s per LCS pass, and the 15
    trees of this case make some 20 passes: by far the longest case here, 47 s measured.)"""
    seqs, ref = _reference(oracle, name)
    engine.upload_seqs(seqs)
    assert engine.orientation_flags().sum() == 0
    bad = []
    for kind in KINDS:
        want = ref[kind & 1][1]
        for mode in MODES:
            _set_mode(monkeypatch, mode)
            try:
                got = engine.mst_prim(kind)
            except famsa_amd.LcsGpuError as e:
                if not re.search("do not converge|added no edge", str(e)):  # the clean end of rounds that lost a vertex's edges; anything else ends here
                    raise
                bad.append((hex(kind), mode, str(e)))
                continue
            if not _same(got, want):
                bad.append((hex(kind), mode, _first_difference(got, want)))
    assert not bad, (name, bad)


class ComputeShards:
    """`parts` contexts on cuda:0 over the same set, context p folding rows [cuts[p], cuts[p+1]) with the fold in the
    LCS launch (LCSGPU_MST_COMPUTE): the block's triangle kept in a device buffer (resident) or never stored."""

    def __init__(self, seqs, parts):
        import torch
        self.torch = torch
        self.n = len(seqs)
        self.parts = parts
        self.cuts = row_cuts(self.n, parts)
        self.engs = []
        for p in range(parts):
            e = famsa_amd.LcsGpu(0)
            self.engs.append(e)
            e.upload_seqs(seqs)
        self.tris = [torch.empty(max(pairs_in_rows(self.cuts[p], self.cuts[p + 1]), 1), dtype=torch.int16, device="cuda:0")
                     for p in range(parts)]
        torch.cuda.synchronize()

    def begin(self, resident, kind):
        for p, e in enumerate(self.engs):
            e.mst_shard_begin(self.tris[p].data_ptr() if resident else None, 2, self.cuts[p], self.cuts[p + 1], kind | MST_COMPUTE)

    def device_flow(self, resident, kind):
        torch = self.torch
        self.begin(resident, kind)
        keys = [torch.zeros(2 * self.n, dtype=torch.int64, device="cuda:0") for _ in self.engs]
        torch.cuda.synchronize()  # torch fills them on ITS stream; the engines write them on theirs
        found, rounds = 0, 0
        while found < self.n - 1:
            assert rounds < 40
            for e, k in zip(self.engs, keys):
                e.mst_shard_best(k.data_ptr())
            for e in self.engs:
                e.sync()
            gathered = torch.cat(keys)
            torch.cuda.synchronize()
            counts = [e.mst_shard_merge(gathered.data_ptr(), self.parts) for e in self.engs]
            assert len(set(counts)) == 1
            found = counts[0]
            rounds += 1
        return [e.mst_shard_finish() for e in self.engs]

    def host_flow(self, resident, kind):
        self.begin(resident, kind)

        def set_components(comp):
            for e in self.engs:
                e.mst_shard_set_components(comp)

        # (sharded_mst_host keeps its own cap on the rounds)
        return sharded_mst_host(self.n, lambda: np.stack([e.mst_shard_best(host=True) for e in self.engs]), lambda k: k,
                                set_components)[0]

    def close(self):
        for e in self.engs:
            e.close()


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("name", SHARD_SHAPES)
def test_row_block_shards_with_the_fold_in_the_launch(oracle, name, parts):
    """1 | LCSGPU_MST_COMPUTE over 2 and 3 contexts: keys exchanged in device memory with the block's triangle given and
    with none (every round recomputes the block), and the host-merge protocol in both forms."""
    seqs, ref = _reference(oracle, name)
    want = ref[1][1]
    sh = ComputeShards(seqs, parts)
    bad = []
    try:
        for resident in (True, False):
            for flow in ("device", "host"):
                try:
                    got = sh.device_flow(resident, 1) if flow == "device" else [sh.host_flow(resident, 1)]
                except (RuntimeError, AssertionError) as e:  # the cap on the rounds, "no convergence", "a round added no edge"
                    if isinstance(e, RuntimeError) and not re.search("converge|added no edge|inside a component", str(e)):
                        raise
                    bad.append((resident, flow, repr(e)))
                    continue
                bad += [(resident, flow, _first_difference(g, want)) for g in got if not _same(g, want)]
    finally:
        sh.close()
    assert not bad, (name, parts, bad)


@pytest.mark.parametrize("name", SHARD_SHAPES)
def test_group_call_that_recomputes(oracle, monkeypatch, name):
    """lcsgpu_multi_mst_prim over two contexts, no triangle anywhere."""
    seqs, ref = _reference(oracle, name)
    grp = famsa_amd.LcsGpuGroup([0, 0])
    try:
        grp.upload_seqs(seqs)
        monkeypatch.setenv("LCSGPU_MST_MODE", "recompute")
        for kind in (1, 0):
            got = grp.mst_prim(kind)
            assert _same(got, ref[kind][1]), (name, kind, _first_difference(got, ref[kind][1]))
    finally:
        grp.close()


@pytest.mark.parametrize("name", SHARD_SHAPES)
def test_row_minima_against_the_reference_distances(engine, oracle, name):
    """lcsgpu_row_minima_dev over the full block and over 3 row blocks: every row's smallest distance among the columns
    before it, and among equals the largest column -- numpy over the reference's matrix."""
    import torch
    seqs, ref = _reference(oracle, name)
    n = len(seqs)
    engine.upload_seqs(seqs)
    below = np.tril(np.ones((n, n), bool), -1)
    for kind in (1, 0):
        D = np.where(below, ref[kind][0], np.inf)
        m = D.min(axis=1)
        j = n - 1 - np.argmax((D == m[:, None])[:, ::-1], axis=1)
        for cuts in ([0, n], row_cuts(n, 3)):
            for r0, r1 in zip(cuts, cuts[1:]):
                tri = torch.empty(max(pairs_in_rows(r0, r1), 1), dtype=torch.int16, device="cuda:0")
                engine.lcs_triangle_dev(r0, r1, tri.data_ptr(), 2)
                out = torch.zeros((r1 - r0, 2), dtype=torch.float64, device="cuda:0")
                torch.cuda.synchronize()  # torch fills on ITS stream; the engine writes `out` on its own
                engine.row_minima_dev(tri.data_ptr(), 2, r0, r1, kind, out.data_ptr(), sync=True)
                d = out[:, 0].cpu().numpy()
                jj = out[:, 1].cpu().numpy().view(np.int64)
                lo = max(r0, 1)  # row 0 has no column before it
                assert (d[lo - r0:].view(np.uint64) == m[lo:r1].view(np.uint64)).all(), (name, kind, r0, r1)
                assert (jj[lo - r0:] == j[lo:r1]).all(), (name, kind, r0, r1)


# ---- the switches a process reads once (LCSGPU_TUNE): a fresh child per setting ----------------------------------------

TUNE_SHAPES = ["zero_last", "duplicates", "ties", "ragged4_sorted", "ragged4_shuffled"]  # b, f, g, j


@pytest.mark.parametrize("tune", ["", "mst_length_bound=0", "mst_keep=0", "mst_crossmul=0"])
def test_each_shortcut_switched_off_alone(oracle, tmp_path, tune):
    """mst_length_bound (tiles let go in the rounds that recompute), mst_keep and mst_crossmul (the passes' shortcuts) are
    read once per process: tests/mst_dump.py in a child of its own per setting -- all on, each off alone -- runs
    `passes` and `recompute` on every set and leaves the edge arrays behind."""
    env = dict(os.environ)
    env.pop("LCSGPU_MST_MODE", None)
    env.pop("LCSGPU_TUNE", None)
    if tune:
        env["LCSGPU_TUNE"] = tune
    jobs = ["%s:%s" % (s, m) for s in TUNE_SHAPES for m in ("passes", "recompute")]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mst_dump.py"), str(tmp_path)] + jobs, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    bad = []
    for job in jobs:
        name, mode = job.split(":")
        flat = np.load(os.path.join(str(tmp_path), "%s_%s.npy" % (name, mode)))
        want = _reference(oracle, name)[1][1][1]
        got = np.zeros(len(flat), dtype=want.dtype)
        got["from"], got["to"], got["dist"] = flat[:, 0], flat[:, 1], flat[:, 2]
        if not _same(got, want):
            bad.append((job, _first_difference(got, want)))
    assert not bad, (tune, bad)


# ---- at size: where the shortcuts are known to fire ---------------------------------------------------------------------

def _pin_lcs(oracle, seqs, sq, rng, count=2000):
    """`count` random pairs of the engine's triangle (as a symmetric square) against the oracle, ref = the larger id."""
    n = len(seqs)
    for i, j in zip(rng.integers(1, n, size=count), rng.integers(0, n, size=count)):
        i, j = int(max(i, j)), int(min(i, j))
        if i != j:
            assert sq[i, j] == oracle.lcs(seqs[i], seqs[j]), (i, j)


def _engine_reference(engine, oracle, seqs, kinds, seed):
    """prim_edges_fast over distances made from engine.lcs_triangle(): the walk and the distances are independent of every
    MST kernel, and the LCS values are pinned to the oracle by 2000 random pairs."""
    lens = np.array([len(s) for s in seqs], np.int64)
    sq = mst_ref.square_lcs(engine.lcs_triangle(), len(seqs))
    _pin_lcs(oracle, seqs, sq, np.random.Generator(np.random.PCG64(seed)))
    return {kind: mst_ref.prim_edges_fast(mst_ref.DistanceRows(sq, lens, kind & 1, oracle)) for kind in kinds}


def test_the_length_bound_at_work_against_the_reference(engine, oracle, monkeypatch, capfd):
    """The 9000-member four-family set of test_the_length_bound_lets_tiles_go_and_changes_nothing (seed 23), in the
    working order, through the rounds that recompute: more than a quarter as many tiles let go as computed (so the
    comparison cannot pass with the bound idle), and the tree of the reference recurrence."""
    rng = np.random.Generator(np.random.PCG64(23))
    fams = []
    for length, members in ((60, 2500), (150, 2500), (420, 2500), (900, 1500)):
        anc = rng.integers(0, 20, size=length, dtype=np.uint8)
        for _ in range(members):
            s = anc.copy()
            m = rng.random(length) < 0.2
            s[m] = rng.integers(0, 20, size=int(m.sum()), dtype=np.uint8)
            fams.append(s[: int(rng.integers(int(length * 0.9), length + 1))].copy())
    order = rng.permutation(len(fams))
    fams = [fams[i] for i in order]
    seqs = [fams[i] for i in seqio.sort_order(fams)]
    engine.upload_seqs(seqs)
    assert engine.orientation_flags().sum() == 0
    want = _engine_reference(engine, oracle, seqs, (1,), seed=1)[1]
    monkeypatch.setenv("LCSGPU_MST_MODE", "recompute")
    monkeypatch.setenv("LCSGPU_MST_COUNTS", "1")
    capfd.readouterr()
    got = engine.mst_prim(1)
    err = capfd.readouterr().err
    line = [l for l in err.splitlines() if "let go by the length bound" in l]
    assert line, err[-1500:]
    print(line[0])
    computed, gone = [int(x) for x in re.findall(r"(\d+) computed, (\d+) let go", line[0])[0]]
    assert gone > computed // 4, line[0]
    assert _same(got, want), _first_difference(got, want)


def test_the_hybrid_against_the_reference(engine, oracle, monkeypatch, capfd):
    """The 4200-member set of test_part_of_the_triangle_resident with room for 60 % of the triangle: resident rows by the
    passes, the rest recomputed per round, against the reference recurrence."""
    rng = np.random.Generator(np.random.PCG64(17))
    [rng.integers(0, 3, size=int(rng.integers(4, 14))) for _ in range(1500)]  # (that test's generator has made its "ties" set first)
    mixed = [rng.integers(0, 20, size=int(l)).astype(np.uint8) for l in rng.integers(20, 700, size=1200)]
    seqs = mixed + seqio.synth_family(3000, 150, seed=5)
    seqs = [seqs[i] for i in seqio.sort_order(seqs)]
    n = len(seqs)
    assert n == 4200
    engine.upload_seqs(seqs)
    assert engine.orientation_flags().sum() == 0
    kinds = (1 | MST_TRIANGLE_ORIENTATION, 0)
    want = _engine_reference(engine, oracle, seqs, kinds, seed=2)
    probe = famsa_amd.LcsGpu(0)  # a fresh context: no result buffer of an earlier call that would already fit
    try:
        probe.upload_seqs(seqs)
        monkeypatch.setenv("LCSGPU_PROFILE", "1")
        monkeypatch.setenv("LCSGPU_FAKE_HBM_GB", "%.6f" % (0.6 * n * (n - 1) / 1e9))
        for kind in kinds:
            capfd.readouterr()
            got = probe.mst_prim(kind)
            err = capfd.readouterr().err
            assert "hybrid" in err, err
            assert _same(got, want[kind]), (kind, _first_difference(got, want[kind]))
    finally:
        probe.close()


# ---- whole blocks of empty sequences in the plain LCS calls -------------------------------------------------------------

@pytest.mark.parametrize("name", ["zero_first", "zero_last"])
def test_plain_lcs_calls_with_whole_blocks_of_empties(engine, oracle, name):
    """A wave or a tile made only of length-0 partners (no 16-residue chunk at all), and refs of length 0 by the block."""
    seqs = mst_shapes.build(name)
    codes, offsets = seqio.pack(seqs)
    n = len(seqs)
    lens = np.array([len(s) for s in seqs])
    empty, full = np.nonzero(lens == 0)[0].astype(np.int32), np.nonzero(lens > 0)[0].astype(np.int32)
    assert len(empty) == 300
    engine.upload_seqs(seqs)
    assert (engine.lcs_triangle(dtype=np.uint32) == oracle.triangle(codes, offsets)).all()
    assert (engine.lcs_triangle() == oracle.triangle(codes, offsets)).all()
    everything = np.arange(n, dtype=np.int32)
    for refs, cols in ((empty, everything), (everything, empty), (full, empty), (empty, full), (empty, empty)):
        want = oracle.rect(codes, offsets, refs, cols)
        assert (engine.lcs_rect(refs, cols, dtype=np.uint32) == want).all()
    first, count = int(empty[0]), len(empty)
    assert (engine.lcs_rect((first, count), (0, n)) == 0).all() and (engine.lcs_rect((0, n), (first, count)) == 0).all()
    ids = np.random.Generator(np.random.PCG64(7)).permutation(n).astype(np.int32)
    assert (engine.lcs_triangle_ids(ids, dtype=np.uint32) == oracle.rect(codes, offsets, ids, ids)[np.tril_indices(n, -1)]).all()
    groups = [ids[:300], empty.copy(), full[::-1].copy(), np.concatenate([empty[:260], full[:5], empty[260:]])]
    got = engine.lcs_triangles_batch(groups, dtype=np.uint32)
    for g, gi in zip(got, groups):
        assert (g == oracle.rect(codes, offsets, gi, gi)[np.tril_indices(len(gi), -1)]).all()


# ---- the command line ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gt", ["sl", "slink"])
def test_cli_with_a_block_of_gap_only_records(tmp_path, gt):
    """-keep-duplicates -gt sl / slink on set b under the three ways to the tree: byte-identical Newick, and the one the
    reference program gives for this file (tests/golden/zero_last_*.dnd, made by oracle/make_golden.py)."""
    path = str(tmp_path / "zero_last.fasta")
    mst_shapes.write_zero_last_fasta(path)
    meta = json.load(open(os.path.join(G, "meta.json")))["zero_last"]
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == meta["fasta_sha256"]
    gold = open(os.path.join(G, "zero_last_%s.dnd" % gt), "rb").read()
    assert hashlib.sha256(gold).hexdigest() == meta["%s_newick_sha256" % gt]
    trees = {}
    for mode in ("passes", "fused", "recompute"):
        out = str(tmp_path / ("%s_%s.dnd" % (gt, mode)))
        env = dict(os.environ)
        env["LCSGPU_MST_MODE"] = mode
        p = subprocess.run([CLI, "-keep-duplicates", "-gt", gt, "-gt_export", path, out], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, env=env, timeout=120)
        assert p.returncode == 0, (mode, p.stderr[-2000:])
        trees[mode] = open(out, "rb").read()
    assert gold.count(b",") == 555
    assert trees["passes"] == gold, "passes"
    assert trees["fused"] == trees["passes"], "fused"
    assert trees["recompute"] == trees["passes"], "recompute"
