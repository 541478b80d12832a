"""Every LCS kernel class at the refs-per-workgroup plans a FULL launch gets.

The planners (refs_per_block_for in csrc/lcs_kernels.hip) give a workgroup the "full complement" of refs R -- up to 32, as
many as fit 32 KB of LDS -- and halve it, in multiples of the register group RG, while the launch would have fewer than 2048
workgroups.  The sets of the quick suite are small, so their launches run at R == RG; what depends on R > RG -- the
register-group loop with its LDS offsets, whole and ragged tiles of fill_tile_masks, odd group counts, the compact triangle
grid with tall tiles, the job tables of the batched planners, the one-wave workgroups with many groups, the quirk kernels
with R > 1, the fused launches' per-(wave, row) records -- runs here, on every one of the 48 pipe and 4 quirk instantiations,
against the oracle.

Nothing large is computed on the CPU: a class has a POOL of 96..128 sequences whose square of LCS values comes from the oracle
once; the uploaded sets and id lists draw from the pool with repetition and the expected values are gathered.  Every test reads
the plan its launch got from the library's trace (LCSGPU_TUNE lcs_plan_trace=1) and asserts it: if planning changes, the test
fails instead of passing at R == RG.  All comparisons are exact."""
import collections
import re

import numpy as np
import pytest

import mst_ref
from famsa_amd.lcsgpu import MST_TRIANGLE_ORIENTATION

pytestmark = pytest.mark.gpu


def _table(rows):
    return {h: r for lo, hi, r in rows for h in range(lo, hi + 1)}


PIPE_H = list(range(1, 33)) + list(range(34, 65, 2))
QUIRK_H = [8, 16, 32, 64]
CLASSES = [("pipe", h) for h in PIPE_H] + [("quirk", h) for h in QUIRK_H]
# the full complement per class, written out (NOT computed the planner's way)
FULL = {"pipe": _table([(1, 8, 32), (9, 10, 24), (11, 12, 20), (13, 16, 16), (17, 18, 14), (19, 20, 12), (21, 24, 10), (25, 32, 8),
                        (33, 36, 7), (37, 42, 6), (43, 50, 5), (51, 64, 4)]),
        "quirk": {8: 32, 16: 16, 32: 8, 64: 4}}
# ... of a fused launch: its records (3200 B) come out of the same 32 KB
FUSED_FULL = {"pipe": _table([(1, 6, 32), (7, 8, 28), (9, 10, 20), (11, 14, 16), (15, 18, 12), (19, 22, 10), (23, 28, 8),
                              (29, 38, 6), (39, 46, 5), (47, 56, 4), (57, 64, 3)]),
              "quirk": {8: 28, 16: 14, 32: 7, 64: 3}}
# contiguous triangles: set sizes at which ceil(n / R) * max(1, ceil((n - 1) / 256) / 2) >= 2048 keeps R
TRI_N = {32: 5900, 28: 5900, 24: 4900, 20: 4600, 16: 4100, 14: 3900, 12: 3600, 10: 3400, 8: 2900, 7: 2900, 6: 2500, 5: 2400,
         4: 2100, 3: 2100}


def _rg(cls):
    kind, h = cls
    return 1 if kind == "quirk" else 4 if h <= 16 else 2 if h <= 32 else 1


def _chain(full, rg):
    """Each step down: max(RG, R / 2 rounded down to a multiple of RG); 24 -> 12 -> 4, 14 -> 6 -> 2, 7 -> 3 -> 1."""
    out = [full]
    while out[-1] > rg:
        out.append(max(rg, out[-1] // 2 // rg * rg))
    return out


def _id(cls):
    return "%s%d" % (cls[0][0], cls[1])


def _seed(cls):
    return 7919 * cls[1] + (1 if cls[0] == "quirk" else 0)


# ---- the plan trace -------------------------------------------------------------------------------------------------------

Launch = collections.namedtuple("Launch", "h quirk fused refs_per_wg threads wgs")
TRACE = re.compile(r"^lcsgpu: lcs launch h=(\d+) quirk=([01]) fused=([01]) refs_per_wg=(\d+) threads=(64|256) wgs=(\d+)$", re.M)


@pytest.fixture
def trace(monkeypatch, capfd):
    """Switches the trace on; trace() returns the launches since the last call."""
    monkeypatch.setenv("LCSGPU_TUNE", "lcs_plan_trace=1")

    def read():
        return [Launch(*map(int, m)) for m in TRACE.findall(capfd.readouterr().err)]

    read()
    return read


def _plan(cls, refs_per_wg, threads=256, fused=0):
    return (cls[1], 1 if cls[0] == "quirk" else 0, fused, refs_per_wg, threads)


# ---- pools ----------------------------------------------------------------------------------------------------------------

def _length_range(cls):
    kind, h = cls
    if kind == "quirk":  # (an aligned word at index >= 1 needs 128 residues)
        return {8: (128, 256), 16: (257, 512), 32: (513, 1024), 64: (1025, 2048)}[h]
    return (32 * (h - 1) + 1, 32 * h) if h <= 32 else (32 * (h - 2) + 1, 32 * h)


def _make_pool(cls):
    """Distinct sequences of the class: both edge lengths, a family (mutated copies of one parent, so that the LCS values spread
    widely) next to unrelated ones, alphabets of 20..22 codes (20 and 21 never match), a few members with runs of code 22 (the
    padding code); quirk classes: an aligned 64-residue homopolymer word at word index >= 1 in every member."""
    rng = np.random.default_rng(_seed(cls))
    lo, hi = _length_range(cls)
    count = 128 if cls[1] <= 16 else 96
    lens = [lo, hi] + [int(x) for x in rng.integers(lo, hi + 1, size=count - 2)]
    parent = rng.integers(0, 20, size=hi).astype(np.uint8)
    seqs, seen = [], set()
    for k, length in enumerate(lens):
        while True:
            letters = int(rng.integers(20, 23))
            s = rng.integers(0, letters, size=length).astype(np.uint8)
            if k % 2 == 0:  # family member
                keep = rng.random(length) >= rng.choice([0.05, 0.2, 0.5])
                s[keep] = parent[:length][keep]
            if k % 9 == 4 and length >= 8:
                a = int(rng.integers(0, length - 4))
                s[a:a + int(rng.integers(3, 40))] = 22
            if cls[0] == "quirk":
                w = int(rng.integers(1, length // 64))
                s[64 * w:64 * w + 64] = rng.choice([3, 7])
            if s.tobytes() not in seen:
                break
        seen.add(s.tobytes())
        seqs.append(s)
    return seqs


def _make_columns():
    """The ragged column pool: 300 sequences of 0..700 residues, the empty one and the chunk / word / block edges included, some
    with long runs of one residue (what a quirk ref's all-ones word needs to meet a carry)."""
    rng = np.random.default_rng(4242)
    lens = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 700] + [int(x) for x in rng.integers(0, 701, size=288)]
    seqs = []
    for k, length in enumerate(lens):
        s = rng.integers(0, int(rng.integers(20, 23)), size=length).astype(np.uint8)
        if k % 10 == 3 and length >= 100:
            a = int(rng.integers(0, length - 90))
            s[a:a + 90] = rng.choice([3, 7])
        seqs.append(s)
    return seqs


COLS = _make_columns()
Pool = collections.namedtuple("Pool", "seqs lens sq rect")
_POOLS = {}


def _pack(seqs):
    offsets = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=offsets[1:])
    return np.concatenate(seqs), offsets


def _pool(oracle, cls):
    """The class's pool with the oracle's values, computed once and read-only: sq[ref, partner] over the pool,
    rect[ref, column] against the column pool."""
    if cls not in _POOLS:
        seqs = _make_pool(cls)
        count = len(seqs)
        codes, offsets = _pack(seqs + COLS)
        both = oracle.rect(codes, offsets, np.arange(count), np.arange(count + len(COLS))).astype(np.uint16)
        sq, rect = both[:, :count].copy(), both[:, count:].copy()
        if cls[0] == "pipe":
            assert (sq == sq.T).all()  # plain refs: the value does not depend on which side is the ref
        sq.flags.writeable = rect.flags.writeable = False
        _POOLS[cls] = Pool(seqs, np.array([len(s) for s in seqs], np.int64), sq, rect)
    return _POOLS[cls]


def _check_flags(engine, cls, count):
    flags = engine.orientation_flags()[:count]
    assert flags.all() if cls[0] == "quirk" else not flags.any()


def _draw(rng, count, n):
    """n pool members, every member at least once."""
    idx = np.concatenate([rng.permutation(count), rng.integers(0, count, size=n - count)])
    rng.shuffle(idx)
    return idx


def _upload_draw(engine, pool, idx):
    engine.upload_seqs([pool.seqs[i] for i in idx])


def _assert_same_rect(got, want, refs_per_wg, what):
    bad = np.argwhere(got != want)
    if len(bad):
        first = ["(ref %d, column %d: tile row %d, lane %d) got %d, want %d" % (r, c, r % refs_per_wg, c % 256, got[r, c], want[r, c])
                 for r, c in bad[:8]]
        pytest.fail("%s: %d of %d values differ; %s" % (what, len(bad), got.size, "; ".join(first)))


def _assert_same_triangle(got, sq, idx, row_begin, row_end, what):
    """got = the packed rows [row_begin, row_end) of the triangle of the set pool[idx]; compared row block by row block."""
    at = 0
    for r0 in range(row_begin, row_end, 512):
        r1 = min(row_end, r0 + 512)
        want = sq[np.ix_(idx[r0:r1], idx[:r1])]
        below = np.arange(r1)[None, :] < np.arange(r0, r1)[:, None]
        want = want[below]
        part = got[at:at + len(want)]
        if (part != want).any():
            k = int(np.flatnonzero(part != want)[0])
            rows, cols = np.nonzero(below)
            pytest.fail("%s: %d values of rows [%d, %d) differ; first at (row %d, column %d): got %d, want %d"
                        % (what, int((part != want).sum()), r0, r1, r0 + rows[k], cols[k], part[k], want[k]))
        at += len(want)
    assert at == len(got)


# ---- 1. rectangles over id lists: every class, every step of the chain ------------------------------------------------------

@pytest.mark.parametrize("cls", CLASSES, ids=_id)
def test_rectangles_at_every_step_of_the_chain(engine, oracle, trace, cls):
    """lcs_rect over id lists: 2 FULL + RG + 1 refs of the class (a ragged last tile with nr % RG != 0 wherever RG > 1) against
    column id lists of the ragged pool, one column count per step of the class's chain -- from ~175 000 columns (three tiles of
    the full complement x 683 column blocks >= 2048 workgroups) down to 256 (R == RG)."""
    pool = _pool(oracle, cls)
    count = len(pool.seqs)
    full, rg = FULL[cls[0]][cls[1]], _rg(cls)
    engine.upload_seqs(pool.seqs + COLS)
    _check_flags(engine, cls, count)
    rng = np.random.default_rng(_seed(cls) + 1)
    n_refs = 2 * full + rg + 1
    refs = np.concatenate([[0, 1], rng.integers(0, count, size=n_refs - 2)]).astype(np.int32)  # (0, 1: the edge lengths)
    dtype = np.uint16 if CLASSES.index(cls) % 2 == 0 else np.uint32
    steps = _chain(full, rg)
    seen = []
    for r in steps:
        # the fewest column blocks that give this step 2048 workgroups (the steps above it then have fewer); RG needs none
        blocks = 1 if r == rg else -(-2048 // -(-n_refs // r))
        n_cols = 256 if blocks == 1 else blocks * 256 - 37
        cols = rng.integers(count, count + len(COLS), size=n_cols).astype(np.int32)
        trace()
        got = engine.lcs_rect(refs, cols, dtype=dtype)
        launches = trace()
        assert len(launches) == 1, launches
        seen.append(launches[0].refs_per_wg)
        assert launches[0][:5] == _plan(cls, r), (launches, r, n_cols)
        _assert_same_rect(got, pool.rect[refs][:, cols - count], r, "%s, %d refs per workgroup, %d columns" % (_id(cls), r, n_cols))
    assert seen == steps


# ---- 2. contiguous triangle: the compact grid at the full complement, every class -------------------------------------------

SPLIT = [("pipe", 13), ("pipe", 21), ("pipe", 44)]  # one class per register group: the triangle in three row blocks as well


@pytest.mark.parametrize("cls", CLASSES, ids=_id)
def test_triangle_at_the_full_complement(engine, oracle, trace, cls):
    """lcs_triangle of n draws from the pool, n large enough for the full complement: the compact grid (tri_prefix, tiles
    across the diagonal) with R rows per tile."""
    pool = _pool(oracle, cls)
    full = FULL[cls[0]][cls[1]]
    n = TRI_N[full]
    idx = _draw(np.random.default_rng(_seed(cls) + 2), len(pool.seqs), n)
    _upload_draw(engine, pool, idx)
    _check_flags(engine, cls, n)
    trace()
    got = engine.lcs_triangle()
    launches = trace()
    assert len(launches) == 1 and launches[0][:5] == _plan(cls, full), launches
    _assert_same_triangle(got, pool.sq, idx, 0, n, _id(cls))
    if cls in SPLIT:
        a, b = n // 3, 2 * n // 3
        while a % full == 0:
            a += 1
        while b % full == 0:
            b += 1
        parts = [engine.lcs_triangle(r0, r1) for r0, r1 in [(0, a), (a, b), (b, n)]]
        assert (np.concatenate(parts) == got).all()


# ---- 3. fused launches at their own full complement ----------------------------------------------------------------------------

# every distinct head of the fused table with every register group it occurs with
FUSED = [("pipe", h) for h in (4, 8, 10, 12, 13, 16, 17, 20, 24, 32, 34, 44, 52, 58, 64)] + [("quirk", h) for h in QUIRK_H]
BOTH_KINDS = [("pipe", 13), ("pipe", 20), ("pipe", 44)]


class _GatheredSquare:
    """Row i of the set's symmetric LCS square in the triangle's orientation (ref = the larger id), gathered from the pool's
    sq[ref, partner] when asked for."""

    def __init__(self, sq, idx):
        self.sq, self.idx, self.ids = sq, idx, np.arange(len(idx))

    def __getitem__(self, i):
        me = self.idx[i]
        return np.where(self.ids < i, self.sq[me][self.idx], self.sq[:, me][self.idx])


def _same_edges(a, b):
    return (a["from"] == b["from"]).all() and (a["to"] == b["to"]).all() and (a["dist"].view(np.uint64) == b["dist"].view(np.uint64)).all()


@pytest.mark.parametrize("cls", FUSED, ids=_id)
def test_fused_launches_at_their_full_complement(engine, oracle, trace, monkeypatch, cls):
    """mst_prim with the fold in the LCS launch -- every round (recompute) or round 0 (fused) -- on a duplicate-heavy set
    (pool repeats: the records' id order decides) against Prim over the gathered oracle square (the quirk classes run in
    the triangle's orientation, ref = the larger id)."""
    pool = _pool(oracle, cls)
    full = FUSED_FULL[cls[0]][cls[1]]
    orientation = MST_TRIANGLE_ORIENTATION if cls[0] == "quirk" else 0
    n = TRI_N[full]
    idx = _draw(np.random.default_rng(_seed(cls) + 3), len(pool.seqs), n)
    _upload_draw(engine, pool, idx)
    _check_flags(engine, cls, n)
    for kind in [1, 0] if cls in BOTH_KINDS else [1]:
        want = mst_ref.prim_edges_fast(mst_ref.DistanceRows(_GatheredSquare(pool.sq, idx), pool.lens[idx], kind, oracle))
        for mode in ("recompute", "fused"):
            monkeypatch.setenv("LCSGPU_MST_MODE", mode)
            trace()
            got = engine.mst_prim(kind | orientation)
            launches = trace()
            assert launches and all(l[:5] == _plan(cls, full, fused=1) for l in launches), (mode, launches)
            assert (len(launches) > 1) == (mode == "recompute"), (mode, launches)
            assert _same_edges(got, want), (cls, kind, mode)


# ---- 4. batched triangles: job tables with full tiles, both workgroup widths ------------------------------------------------------

BATCH = [("pipe", 3), ("pipe", 9), ("pipe", 13), ("pipe", 17), ("pipe", 21), ("pipe", 34), ("pipe", 44), ("pipe", 64), ("quirk", 8)]


def _list_sizes(rng, lo, hi, mid_lo, mid_hi, full, want_refs):
    """Ragged list sizes in [lo, hi], most of them in [mid_lo, mid_hi]: neither the members nor the refs (members - 1) of a list
    are a multiple of the tile height, so every list ends inside a tile; as many lists as give want_refs refs."""
    def ok(m):
        return full == 1 or (m % full and (m - 1) % full)
    sizes = [m for m in (lo, lo + 1, hi, hi - 1) if ok(m)]
    refs = sum(m - 1 for m in sizes)
    while refs < want_refs:
        m = int(rng.integers(mid_lo, mid_hi + 1))
        if ok(m):
            sizes.append(m)
            refs += m - 1
    rng.shuffle(sizes)
    return sizes


@pytest.mark.parametrize("width", ["narrow", "wide"])
@pytest.mark.parametrize("cls", BATCH, ids=_id)
def test_batched_triangles_with_full_tiles(engine, oracle, trace, cls, width):
    """lcsgpu_lcs_triangles_batch: enough id lists for ceil(refs / R) >= 2048, so the job table is cut into tiles of the full
    complement -- lists of 2..192 members (one-wave workgroups for plain refs) and of 193..600 members (256 threads)."""
    pool = _pool(oracle, cls)
    count = len(pool.seqs)
    full = FULL[cls[0]][cls[1]]
    engine.upload_seqs(pool.seqs)
    _check_flags(engine, cls, count)
    rng = np.random.default_rng(_seed(cls) + (4 if width == "narrow" else 5))
    if width == "narrow":
        sizes = _list_sizes(rng, 2, 192, 40, 75, full, 2049 * full)
    else:
        sizes = _list_sizes(rng, 193, 600, 330, 470, full, 2049 * full)
    rgs = {m % _rg(cls) for m in sizes}
    assert rgs == set(range(_rg(cls)))  # list ends at every position inside a register group
    lists = [rng.integers(0, count, size=m).astype(np.int32) for m in sizes]
    trace()
    got = engine.lcs_triangles_batch(lists)
    launches = trace()
    threads = 64 if width == "narrow" and cls[0] == "pipe" else 256  # (orientation-sensitive refs: 256 only)
    assert len(launches) == 1 and launches[0][:5] == _plan(cls, full, threads=threads), launches
    for g, ids in enumerate(lists):
        want = pool.sq[np.ix_(ids, ids)][np.tril_indices(len(ids), -1)]
        bad = np.flatnonzero(got[g] != want)
        if len(bad):
            rows, cols = np.tril_indices(len(ids), -1)
            k = int(bad[0])
            pytest.fail("%s %s: list %d of %d members: %d values differ; first at (member %d, member %d): got %d, want %d"
                        % (_id(cls), width, g, len(ids), len(bad), rows[k], cols[k], got[g][k], want[k]))


# ---- 5. batched seed rectangles ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", [4, 34])
def test_batched_seed_rectangles_at_the_full_complement(engine, oracle, trace, h):
    """lcsgpu_assign_seeds_batch: two evaluations of ~100 seeds of the class and ~80 000 columns each (ceil(seeds / R) x column
    blocks per piece >= 2048) against the host sweep -- the first seed's row, then strict '<' in seed order -- over a table of the
    oracle's float distances per (pool seed, uploaded column)."""
    cls = ("pipe", h)
    pool = _pool(oracle, cls)
    count = len(pool.seqs)
    full = FULL["pipe"][h]
    seqs = pool.seqs + COLS
    engine.upload_seqs(seqs)
    lens = [len(s) for s in seqs]
    lcs = np.concatenate([pool.sq, pool.rect], axis=1)
    fn = oracle.lib.oracle_dist_indel075_f32
    table = np.array([[fn(int(lcs[s, c]), lens[s], lens[c]) for c in range(len(seqs))] for s in range(count)], np.float32)
    rng = np.random.default_rng(_seed(cls) + 6)
    seeds = [rng.integers(0, count, size=m).astype(np.int32) for m in (101, 103)]  # (neither a multiple of R = 32 / 7)
    cols = [rng.integers(0, len(seqs), size=m).astype(np.int32) for m in (80000, 81001)]
    trace()
    got_d, got_a = engine.assign_seeds_batch(seeds, cols, kind=1)
    launches = trace()
    assert len(launches) == 1 and launches[0][:5] == _plan(cls, full), launches
    for g in range(2):
        d = table[seeds[g]][:, cols[g]]
        want_a = d.argmin(axis=0).astype(np.int32)  # the first of equal minima: what strict '<' in seed order keeps
        want_d = d[want_a, np.arange(d.shape[1])]
        assert (got_a[g] == want_a).all(), (h, g, int((got_a[g] != want_a).sum()))
        assert (got_d[g].view(np.uint32) == want_d.view(np.uint32)).all(), (h, g)


def test_the_trace_is_silent_when_unset(engine, oracle, capfd, monkeypatch):
    """Without lcs_plan_trace (or with it at 0) a launch writes nothing."""
    pool = _pool(oracle, ("pipe", 3))
    engine.upload_seqs(pool.seqs)
    for value in (None, "lcs_plan_trace=0"):
        if value is None:
            monkeypatch.delenv("LCSGPU_TUNE", raising=False)
        else:
            monkeypatch.setenv("LCSGPU_TUNE", value)
        capfd.readouterr()
        got = engine.lcs_rect((0, 8), (0, len(pool.seqs)))
        assert capfd.readouterr().err == ""
        assert (got == pool.sq[:8]).all()
