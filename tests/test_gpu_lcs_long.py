"""Class 0 of the LCS engine -- lcs_long_kernel<QUIRK, FUSE> of csrc/lcs_kernels.hip, the segmented kernel for refs beyond 2048
residues -- against the oracle: the sibling of test_gpu_lcs_plans.py, whose trace fixture and comparison helpers serve here too.

What the kernel does by hand and what pins it here: a ref is cut into passes of 16 words and closed by an 8- or a 16-word pass
(every word count 33..48 and 49 / 64 / 65 / 80 / 81 / 96, both edge lengths: every n_words mod 16, both last-pass widths, every
count of zero-mask padding words, 3 to 6 passes); carries between passes go through a per-lane stream in global scratch, indexed
by workgroup and chunk and strided by the SET's longest sequence (a 20 000-residue bystander that no call names), read a chunk
ahead and reused by all 8 refs of a workgroup (a 6-pass ref directly before a 3-pass ref); orientation-sensitive refs take a
literal 64-bit branch (an aligned homopolymer word at the last word of a pass, the first of the next, both, ...); the 2-D grid is
remapped by block_coords (several column blocks, several ref tiles, a ragged last tile); a launch whose carry scratch would
exceed its budget is cut into ref-tile slices (LCSGPU_TUNE long_carry_mb).

Every test reads the launch trace (LCSGPU_TUNE lcs_plan_trace=1) and asserts h=0 with the quirk= and fused= it expects and
refs_per_wg=8: if routing changes, the test fails instead of passing through another kernel.  The oracle's values are computed
once per module (a few seconds) and kept read-only; uploaded sets and id lists draw from the pools.  All comparisons are exact."""
import collections

import numpy as np
import pytest

import mst_ref
from famsa_amd.lcsgpu import MST_TRIANGLE_ORIENTATION
from test_gpu_lcs_plans import _GatheredSquare, _assert_same_rect, _assert_same_triangle, _draw, _pack, _same_edges, trace  # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = ["plain", "quirk"]
PLAIN_WORDS = list(range(33, 49)) + [49, 64, 65, 80, 81, 96]
QUIRK_WORDS = [33, 40, 41, 48, 49, 70]
LAST_FULL = "the last full word"
# word indices of the aligned 64-residue homopolymer: 15 | 16 and 31 | 32 are the last word of one pass and the first of the next
QUIRK_AT = [(1,), (15,), (16,), (15, 16), (31,), (32,), (31, 32), LAST_FULL, (1, 16, 32)]
REFS_PER_WG = 8  # refs_per_block(0, ...): the long kernel walks its refs one after another
SHORT = 24  # the first SHORT run-carrying and the first SHORT other columns of 64..2048 residues double as short refs


def _passes(n_words):
    """Passes of a ref of n_words words: 16 words each, the last one 8 or 16."""
    return -(-n_words // 16)


def _words(length):
    return -(-length // 64)


def _family_member(rng, parent, length, k):
    """_make_pool's recipe of test_gpu_lcs_plans.py: an alphabet of 20..22 codes, every other member a mutated copy of the
    parent, a few members with a run of code 22."""
    s = rng.integers(0, int(rng.integers(20, 23)), size=length).astype(np.uint8)
    if k % 2 == 0:
        keep = rng.random(length) >= rng.choice([0.05, 0.2, 0.5])
        s[keep] = parent[:length][keep]
    if k % 9 == 4:
        a = int(rng.integers(0, length - 40))
        s[a:a + int(rng.integers(3, 40))] = 22
    return s


def _make_plain():
    rng = np.random.default_rng(20480)
    parent = rng.integers(0, 20, size=64 * 96).astype(np.uint8)
    lens = [length for w in PLAIN_WORDS for length in (64 * (w - 1) + 1, 64 * w)]
    return [_family_member(rng, parent, length, k) for k, length in enumerate(lens)]


def _make_quirk():
    """Every index set of QUIRK_AT at every word count of QUIRK_WORDS.  Lengths: 64 w where a homopolymer word is the ref's last
    word, 64 (w - 1) + 17 for LAST_FULL (word w - 2 then, a partial word behind it), else one of the two in turn."""
    rng = np.random.default_rng(20481)
    parent = rng.integers(0, 20, size=64 * 70).astype(np.uint8)
    seqs = []
    for w in QUIRK_WORDS:
        for at in QUIRK_AT:
            k = len(seqs)
            if at == LAST_FULL:
                length, at = 64 * (w - 1) + 17, (w - 2,)
            else:
                length = 64 * w if max(at) == w - 1 or k % 2 else 64 * (w - 1) + 1 + int(rng.integers(0, 63))
            s = _family_member(rng, parent, length, k)
            for i in at:
                assert 1 <= i and 64 * i + 64 <= length
                s[64 * i:64 * i + 64] = rng.choice([3, 7])
            seqs.append(s)
    return seqs


def _make_columns():
    """The partners: the chunk / word / block edges, the longest ones longer than every ref, ~280 more of 0..700 residues; every
    fifth carries a 90-residue run of code 3 or 7 (what an all-ones word of a quirk ref needs to meet a carry), two of 3000
    residues carry 150-residue runs every 400 residues."""
    rng = np.random.default_rng(20482)
    lens = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 700, 2048, 2049, 5000, 6200] + [int(x) for x in rng.integers(0, 701, size=284)]
    seqs = []
    for k, length in enumerate(lens):
        s = rng.integers(0, int(rng.integers(20, 23)), size=length).astype(np.uint8)
        if k % 5 == 3 and length >= 100:
            a = int(rng.integers(0, length - 90))
            s[a:a + 90] = rng.choice([3, 7])
        seqs.append(s)
    for _ in range(2):
        s = rng.integers(0, 21, size=3000).astype(np.uint8)
        for a in range(int(rng.integers(0, 200)), 3000 - 150, 400):
            s[a:a + 150] = rng.choice([3, 7])
        seqs.append(s)
    return seqs


PLAIN, QUIRK, COLS = _make_plain(), _make_quirk(), _make_columns()
LONG = PLAIN + QUIRK
N_PLAIN, N_QUIRK, N_LONG, N_COLS = len(PLAIN), len(QUIRK), len(PLAIN) + len(QUIRK), len(COLS)
assert (N_PLAIN, N_QUIRK, N_COLS) == (44, 54, 302)
assert len({s.tobytes() for s in LONG}) == N_LONG
Pool = collections.namedtuple("Pool", "seqs lens sq rect")
_ORACLE = {}


def _has_run(s):
    return len(s) >= 90 and bool((np.convolve(s[1:] == s[:-1], np.ones(89, np.int64)) == 89).any())


def _short_ids():
    """Columns of 64..2048 residues that double as short refs in the mixed call: the first SHORT with a long run, the first SHORT
    without one (positions in COLS)."""
    runs = [k for k, s in enumerate(COLS) if 128 <= len(s) <= 2048 and _has_run(s)][:SHORT]
    others = [k for k, s in enumerate(COLS) if 64 <= len(s) <= 2048 and not _has_run(s)][:SHORT]
    assert len(runs) == len(others) == SHORT
    return np.array(runs + others, np.int32)


def _values(oracle):
    """The oracle's values, computed once and read-only: long[ref, partner] for every long ref (the plain pool, then the quirk
    pool) against LONG + COLS, short[k, partner] for the columns _short_ids() against COLS, and swapped[column, quirk ref] = the
    quirk pool as PARTNERS of the columns."""
    if not _ORACLE:
        codes, offsets = _pack(LONG + COLS)
        long = oracle.rect(codes, offsets, np.arange(N_LONG), np.arange(N_LONG + N_COLS)).astype(np.uint16)
        short = oracle.rect(codes, offsets, N_LONG + _short_ids(), np.arange(N_LONG, N_LONG + N_COLS)).astype(np.uint16)
        swapped = oracle.rect(codes, offsets, np.arange(N_LONG, N_LONG + N_COLS), np.arange(N_PLAIN, N_LONG)).astype(np.uint16)
        plain_sq = long[:N_PLAIN, :N_PLAIN]
        assert (plain_sq == plain_sq.T).all()  # plain refs: the value does not depend on which side is the ref
        # the quirk pool stays what it is here for: every member's value against some column depends on the orientation
        differs = (long[N_PLAIN:, N_LONG:] != swapped.T).any(axis=1)
        assert differs.all(), np.flatnonzero(~differs).tolist()
        for a in (long, short, swapped):
            a.flags.writeable = False
        _ORACLE.update(long=long, short=short, swapped=swapped)
    return _ORACLE


def _pool(oracle, kind):
    """One pool as test_gpu_lcs_plans.py's Pool: sq[ref, partner] over the pool, rect[ref, column] against COLS."""
    v = _values(oracle)["long"]
    lo, hi = (0, N_PLAIN) if kind == "plain" else (N_PLAIN, N_LONG)
    return Pool(LONG[lo:hi], np.array([len(s) for s in LONG[lo:hi]], np.int64), v[lo:hi, lo:hi], v[lo:hi, N_LONG:])


def _check_flags(engine, kind, count):
    flags = engine.orientation_flags()[:count]
    assert flags.all() if kind == "quirk" else not flags.any()


def _long_plan(kind, fused=0):
    return (0, 1 if kind == "quirk" else 0, fused, REFS_PER_WG, 256)


def _slices(n_refs, n_col_blocks, max_len, carry_mb):
    """Ref-tile rows of every launch of one class 0 call, as DESIGN 3.3 documents the planner: a workgroup's carry stream holds one
    16-bit word per lane (256) and 16-residue chunk of the set's longest sequence, a launch gets as many tile rows (of 8 refs, times
    the call's column blocks) as fit long_carry_mb MB -- one at least."""
    per_workgroup = -(-max_len // 16) * 256 * 2
    step = max(1, (carry_mb << 20) // per_workgroup // n_col_blocks)
    tile_rows = -(-n_refs // REFS_PER_WG)
    return [min(step, tile_rows - y) for y in range(0, tile_rows, step)]


def _assert_class0(launches, kind, wgs, fused=0):
    """One class 0 launch per entry of wgs, in order, and nothing else."""
    assert [l[:5] for l in launches] == [_long_plan(kind, fused)] * len(wgs) and [l.wgs for l in launches] == list(wgs), (launches, wgs)


def _ref_order(pool, rng, n_refs):
    """n_refs pool members: the one with the most passes directly before one with 3 passes (both in the first workgroup, which
    reuses its carry stream from ref to ref), both edge lengths of the pool, then draws."""
    passes = np.array([_passes(_words(n)) for n in pool.lens])
    most = int(np.flatnonzero(passes == passes.max())[-1])
    three = int(np.flatnonzero(passes == 3)[0])
    assert passes[most] >= 5 and pool.lens[most] > pool.lens[three]
    rest = rng.permutation(len(pool.seqs))[:n_refs - 4]
    return np.concatenate([[most, three, int(pool.lens.argmin()), int(pool.lens.argmax())], rest]).astype(np.int32)


# ---- 1. rectangles over id lists -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bystander", [False, True], ids=["set", "bystander"])
@pytest.mark.parametrize("kind", KINDS)
def test_rectangles_over_id_lists(engine, oracle, trace, kind, bystander):
    """lcs_rect over id lists: 19 refs (three tiles, the last of 3) against 600 columns drawn with repetition (3 column blocks,
    ragged lanes in a wave, lanes beyond n_cols), uint16 and uint32.  bystander: a 20 000-residue sequence that no call names is
    in the set, so the stride of the carry streams (the set's longest sequence) is far from any chunk count of the call."""
    pool = _pool(oracle, kind)
    count = len(pool.seqs)
    rng = np.random.default_rng(301 + KINDS.index(kind))
    extra = [rng.integers(0, 20, size=20000).astype(np.uint8)] if bystander else []
    engine.upload_seqs(pool.seqs + COLS + extra)
    _check_flags(engine, kind, count)
    refs = _ref_order(pool, rng, 19)
    cols = rng.integers(count, count + N_COLS, size=600).astype(np.int32)
    cols[:16] = count + np.arange(16)  # (the edge lengths, 5000 and 6200 among them)
    want = pool.rect[refs][:, cols - count]
    for dtype in (np.uint16, np.uint32):
        trace()
        got = engine.lcs_rect(refs, cols, dtype=dtype)
        _assert_class0(trace(), kind, [3 * 3])
        assert got.dtype == dtype
        _assert_same_rect(got, want, REFS_PER_WG, "%s, %s, bystander %s" % (kind, dtype.__name__, bystander))


# ---- 2. contiguous rectangle --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_contiguous_rectangle(engine, oracle, trace, kind):
    """lcs_rect((a, b), (c, d)) with a > 0: ref_begin / col_begin instead of id tables; the columns are the rest of the pool
    (partners as long as the refs) and 270 of the column pool."""
    pool = _pool(oracle, kind)
    count = len(pool.seqs)
    engine.upload_seqs(pool.seqs + COLS)
    _check_flags(engine, kind, count)
    a, b, c, d = 3, count - 5, 7, count - 7 + 270
    trace()
    got = engine.lcs_rect((a, b), (c, d))
    _assert_class0(trace(), kind, [-(-d // 256) * -(-b // REFS_PER_WG)])
    want = np.concatenate([pool.sq, pool.rect], axis=1)[a:a + b, c:c + d]
    _assert_same_rect(got, want, REFS_PER_WG, kind)


# ---- 3. contiguous triangle ---------------------------------------------------------------------------------------------------

TRI_N = 333


def _triangle_wgs(n, carry_mb=2048, max_len=0):
    """Workgroups of the launches of lcs_triangle() over n sequences: a 2-D grid over the columns below the last row."""
    col_blocks = -(-(n - 1) // 256)
    return [col_blocks * rows for rows in _slices(n, col_blocks, max_len, carry_mb)] if max_len else [col_blocks * -(-n // REFS_PER_WG)]


@pytest.mark.parametrize("kind", KINDS)
def test_contiguous_triangle(engine, oracle, trace, kind):
    """lcs_triangle of 333 draws of the pool (2 column blocks: block_is_above_diagonal both skips and keeps blocks), whole and
    in three row ranges (row_begin > 0: out_offset), and lcs_triangle_ids over a shuffled id list (ref_rows)."""
    pool = _pool(oracle, kind)
    rng = np.random.default_rng(311 + KINDS.index(kind))
    n = TRI_N
    idx = _draw(rng, len(pool.seqs), n)
    engine.upload_seqs([pool.seqs[i] for i in idx])
    _check_flags(engine, kind, n)
    trace()
    got = engine.lcs_triangle()
    _assert_class0(trace(), kind, _triangle_wgs(n))
    _assert_same_triangle(got, pool.sq, idx, 0, n, kind)
    a, b = 101, 250  # (neither a multiple of the tile height)
    parts = []
    for r0, r1 in [(0, a), (a, b), (b, n)]:
        trace()
        parts.append(engine.lcs_triangle(r0, r1))
        _assert_class0(trace(), kind, [-(-(r1 - 1) // 256) * -(-(r1 - r0) // REFS_PER_WG)])
    assert (np.concatenate(parts) == got).all()
    ids = rng.permutation(n)[:300].astype(np.int32)
    trace()
    got = engine.lcs_triangle_ids(ids)
    launches = trace()
    assert launches and all(l[:5] == _long_plan(kind) for l in launches), launches
    _assert_same_triangle(got, pool.sq, idx[ids], 0, len(ids), kind + ", id list")


# ---- 4. long, short and orientation-sensitive refs in one call -------------------------------------------------------------------

@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_mixed_call(engine, oracle, trace, order):
    """One id list with refs of class 0 (plain and orientation-sensitive) and short refs of both kinds: the class 0 launches run
    beside the others, every ref's row lands where the list puts it."""
    v = _values(oracle)
    engine.upload_seqs(LONG + COLS)
    flags = engine.orientation_flags()
    assert not flags[:N_PLAIN].any() and flags[N_PLAIN:N_LONG].all()
    short = _short_ids()
    short_flags = flags[N_LONG + short]
    assert short_flags[:SHORT].sum() >= 4 and not short_flags[SHORT:].any()  # short orientation-sensitive refs, and plain ones
    rng = np.random.default_rng(321)
    long_refs = np.concatenate([rng.permutation(N_PLAIN)[:13], N_PLAIN + rng.permutation(N_QUIRK)[:11]])
    refs = np.concatenate([long_refs, N_LONG + short]).astype(np.int32)
    want_rows = np.concatenate([v["long"][long_refs][:, N_LONG:], v["short"]])
    by_length = np.argsort([len((LONG + COLS)[i]) for i in refs], kind="stable")
    order_of = by_length if order == "sorted" else rng.permutation(len(refs))
    refs, want_rows = refs[order_of], want_rows[order_of]
    cols = rng.integers(0, N_COLS, size=500).astype(np.int32)
    trace()
    got = engine.lcs_rect(refs, N_LONG + cols)
    launches = trace()
    long_launches = [l for l in launches if l.h == 0]
    assert sorted(l[:5] for l in long_launches) == [_long_plan("plain"), _long_plan("quirk")], launches
    assert sorted(l.wgs for l in long_launches) == [2 * 2, 2 * 2], launches  # 13 and 11 refs: two tiles each, 2 column blocks
    assert {l.quirk for l in launches if l.h > 0} == {0, 1}, launches
    _assert_same_rect(got, want_rows[:, cols], REFS_PER_WG, order)


# ---- 5. fused launches ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_fused_launches(engine, oracle, trace, monkeypatch, kind):
    """mst_prim with the fold in the LCS launch -- every round (recompute) or round 0 (fused) -- on ~300 draws of the pool (pool
    repeats: the records' id order decides) against Prim over the gathered oracle square; the quirk pool runs in the triangle's
    orientation (ref = the larger id)."""
    pool = _pool(oracle, kind)
    orientation = MST_TRIANGLE_ORIENTATION if kind == "quirk" else 0
    n = 301
    idx = _draw(np.random.default_rng(331 + KINDS.index(kind)), len(pool.seqs), n)
    engine.upload_seqs([pool.seqs[i] for i in idx])
    _check_flags(engine, kind, n)
    for dist in (1, 0):
        want = mst_ref.prim_edges_fast(mst_ref.DistanceRows(_GatheredSquare(pool.sq, idx), pool.lens[idx], dist, oracle))
        for mode in ("recompute", "fused"):
            monkeypatch.setenv("LCSGPU_MST_MODE", mode)
            trace()
            got = engine.mst_prim(dist | orientation)
            launches = trace()
            assert launches and all(l[:5] == _long_plan(kind, fused=1) for l in launches), (mode, launches)
            assert (len(launches) > 1) == (mode == "recompute"), (mode, launches)
            assert _same_edges(got, want), (kind, dist, mode)


# ---- 6. launches cut into ref-tile slices -----------------------------------------------------------------------------------------

def _tune(monkeypatch, setting):
    monkeypatch.setenv("LCSGPU_TUNE", "lcs_plan_trace=1" + ("," + setting if setting else ""))


@pytest.mark.parametrize("refs_as", ["id list", "range"])
@pytest.mark.parametrize("kind", KINDS)
def test_sliced_rectangle(engine, oracle, trace, monkeypatch, kind, refs_as):
    """long_carry_mb=1 on the set with the 6200-residue column: a rectangle of 40 refs x 2 column blocks runs as several class 0
    launches, each over the next tile rows of the ref list (the id and row tables, or ref_begin and row0, advance); with a
    40 000-residue bystander a workgroup's stream is larger than the budget and every tile row is a launch of its own.  The
    values are those of the unsliced call and the oracle's."""
    pool = _pool(oracle, kind)
    count = len(pool.seqs)
    rng = np.random.default_rng(341 + KINDS.index(kind))
    refs = (2, 40) if refs_as == "range" else rng.permutation(count)[:40].astype(np.int32)
    rows = np.arange(2, 42) if refs_as == "range" else refs
    cols = rng.integers(count, count + N_COLS, size=300).astype(np.int32)
    cols[:16] = count + np.arange(16)
    want = pool.rect[rows][:, cols - count]
    for extra, max_len in (([], 6200), ([np.full(40000, 21, np.uint8)], 40000)):
        engine.upload_seqs(pool.seqs + COLS + extra)
        assert int(engine.lengths.max()) == max_len
        sliced = _slices(40, 2, max_len, 1)
        assert len(sliced) >= 3 and sum(sliced) == 5
        if extra:
            assert sliced == [1] * 5  # 2500 chunks x 512 B: more than 1 MB
        _tune(monkeypatch, None)
        trace()
        whole = engine.lcs_rect(refs, cols)
        _assert_class0(trace(), kind, [2 * 5])
        _tune(monkeypatch, "long_carry_mb=1")
        trace()
        got = engine.lcs_rect(refs, cols)
        _assert_class0(trace(), kind, [2 * r for r in sliced])
        assert (got == whole).all()
        _assert_same_rect(got, want, REFS_PER_WG, "%s, %s, longest %d" % (kind, refs_as, max_len))


@pytest.mark.parametrize("kind", KINDS)
def test_sliced_triangle(engine, oracle, trace, monkeypatch, kind):
    """The contiguous triangle with long_carry_mb=1: row0 advances with the slices, whole and from a row_begin > 0."""
    pool = _pool(oracle, kind)
    rng = np.random.default_rng(351 + KINDS.index(kind))
    n = TRI_N
    idx = _draw(rng, len(pool.seqs), n)
    engine.upload_seqs([pool.seqs[i] for i in idx])
    max_len = int(pool.lens.max())
    wgs = _triangle_wgs(n, 1, max_len)
    assert len(wgs) >= 3
    _tune(monkeypatch, None)
    trace()
    whole = engine.lcs_triangle()
    _assert_class0(trace(), kind, _triangle_wgs(n))
    _tune(monkeypatch, "long_carry_mb=1")
    trace()
    got = engine.lcs_triangle()
    _assert_class0(trace(), kind, wgs)
    assert (got == whole).all()
    _assert_same_triangle(got, pool.sq, idx, 0, n, kind)
    r0 = 203
    trace()
    part = engine.lcs_triangle(r0, n)
    _assert_class0(trace(), kind, [2 * r for r in _slices(n - r0, 2, max_len, 1)])
    assert (part == whole[r0 * (r0 - 1) // 2:]).all()
