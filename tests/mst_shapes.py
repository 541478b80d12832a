"""Test infrastructure: the degenerate sequence sets of test_mst_ref.py / test_gpu_mst_reference.py, by name, with fixed
seeds -- whole blocks of empty sequences, LCS-0 pairs at positive lengths, exact duplicates, ties that only the ids
settle, prefixes of one sequence, sizes around the 256-column tile, families far apart in length, the longest sequence
the 16-bit records hold.  Every set is returned in UPLOAD order (no sorting, no de-duplication on the way to the engine).
Nothing in famsa_amd/ imports this."""
import numpy as np

from famsa_amd import seqio

UNKNOWN = 22  # the code that matches nothing, not even itself


def _random(rng, lo, hi, count, letters=20):
    """`count` sequences over `letters` symbols, lengths uniform in [lo, hi]."""
    return [rng.integers(0, letters, size=int(l)).astype(np.uint8) for l in rng.integers(lo, hi + 1, size=count)]


def _empties(count):
    return [np.zeros(0, np.uint8) for _ in range(count)]


def _ragged4(rng):
    fams = []
    for length in (30, 150, 420, 900):
        anc = rng.integers(0, 20, size=length, dtype=np.uint8)
        for _ in range(150):
            s = anc.copy()
            m = rng.random(length) < 0.2
            s[m] = rng.integers(0, 20, size=int(m.sum()), dtype=np.uint8)
            fams.append(s[: int(rng.integers(int(length * 0.9), length + 1))].copy())
    return fams + _random(rng, 2100, 3000, 4)


def build(name):
    """The set `name` as a list of uint8 code arrays in upload order."""
    if name == "zero_first":       # a: ids 0..255 are a whole column block of empties
        rng = np.random.Generator(np.random.PCG64(101))
        return _empties(300) + _random(rng, 1, 60, 300)
    if name == "zero_last":        # b: FAMSA's working order; ids 256..511 are a whole column block of empties
        rng = np.random.Generator(np.random.PCG64(102))
        seqs = _random(rng, 33, 90, 256)
        return [seqs[i] for i in seqio.sort_order(seqs)] + _empties(300)
    if name == "zero_scattered":   # c
        rng = np.random.Generator(np.random.PCG64(103))
        seqs = _random(rng, 1, 60, 600)
        return [np.zeros(0, np.uint8) if i % 7 == 0 else s for i, s in enumerate(seqs)]
    if name == "zero_only":        # d: every distance is the huge one, the ids decide everything
        return _empties(300)
    if name == "zero_and_unknown":  # d
        rng = np.random.Generator(np.random.PCG64(104))
        return _empties(40) + [np.full(int(l), UNKNOWN, np.uint8) for l in rng.integers(1, 41, size=40)]
    if name == "allx":             # e: LCS 0 at positive lengths
        rng = np.random.Generator(np.random.PCG64(105))
        return [np.full(int(l), UNKNOWN, np.uint8) for l in rng.integers(1, 80, size=300)] + _random(rng, 1, 60, 300)
    if name == "duplicates":       # f: distance 0, ties
        rng = np.random.Generator(np.random.PCG64(106))
        seqs = _random(rng, 20, 120, 200) * 3
        return [seqs[i].copy() for i in rng.permutation(len(seqs))]
    if name == "ties":             # g
        rng = np.random.Generator(np.random.PCG64(107))
        return _random(rng, 3, 11, 600, letters=3)
    if name == "prefixes":         # h
        rng = np.random.Generator(np.random.PCG64(108))
        anc = rng.integers(0, 20, size=420, dtype=np.uint8)
        return [anc[: int(l)].copy() for l in rng.integers(40, 421, size=500)]
    if name.startswith("n") and name[1:].isdigit():  # i
        n = int(name[1:])
        return _random(np.random.Generator(np.random.PCG64(1000 + n)), 5, 40, n)
    if name == "ragged4_sorted":   # j
        seqs = _ragged4(np.random.Generator(np.random.PCG64(110)))
        return [seqs[i] for i in seqio.sort_order(seqs)]
    if name == "ragged4_shuffled":
        rng = np.random.Generator(np.random.PCG64(110))
        seqs = _ragged4(rng)
        return [seqs[i] for i in rng.permutation(len(seqs))]
    if name == "maxlen":           # k: 65535 is the longest length a 16-bit record holds
        rng = np.random.Generator(np.random.PCG64(111))
        return _random(rng, 20, 300, 60) + [rng.integers(0, 20, size=65535).astype(np.uint8),
                                            rng.integers(0, 20, size=65534).astype(np.uint8)]
    raise KeyError(name)


def write_zero_last_fasta(path):
    """Set b as a FASTA: the empty sequences are gap-only records (the reader keeps them as length 0)."""
    with open(path, "w") as f:
        for i, s in enumerate(build("zero_last")):
            f.write(">s%d\n%s\n" % (i, "".join(seqio.ALPHABET[c] for c in s) if len(s) else "-"))


CPU_SHAPES = ["zero_first", "zero_last", "zero_scattered", "zero_only", "zero_and_unknown", "allx", "duplicates", "ties",
              "prefixes"]                                                        # a - h
GPU_SHAPES = CPU_SHAPES + ["n2", "n3", "n255", "n256", "n257", "ragged4_sorted", "ragged4_shuffled", "maxlen"]  # a - k
