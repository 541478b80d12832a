"""ctypes binding of libfamsa_host.so -- the C++ host layer above the C-ABI (working order, guide-tree
builders over GPU LCS, Newick / CSV writers) -- plus two convenience functions for Python callers."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_SO = os.path.join(_HERE, "libfamsa_host.so")
CLI = os.path.join(_HERE, "famsa-gpu")
DIST = {"indel_div_lcs": 0, "indel075_div_lcs": 1}


class Host:
    def __init__(self):
        from .lcsgpu import load_library
        load_library()  # resolves liblcsgpu.so (and lets torch's HIP runtime load first)
        if not os.path.exists(HOST_SO):
            raise RuntimeError(f"{HOST_SO} not found: build it with `make -C famsa_amd/host`")
        lib = C.CDLL(HOST_SO)
        lib.famsa_host_last_error.restype = C.c_char_p
        lib.famsa_host_tree_from_matrix.restype = C.c_long
        heur = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int]
        lib.famsa_host_tree_from_matrix.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int, *heur,
                                                    C.c_char_p, C.c_long]
        lib.famsa_host_tree_from_matrix_ex.restype = C.c_long
        lib.famsa_host_tree_from_matrix_ex.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int, *heur, C.c_int,
                                                       C.c_uint32, C.c_char_p, C.c_char_p, C.c_long]
        lib.famsa_host_dist_export_from_matrix.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                           C.c_char_p]
        lib.famsa_host_tree_gpu.restype = C.c_long
        lib.famsa_host_tree_gpu.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, *heur, C.c_char_p,
                                            C.c_long]
        lib.famsa_host_trees_gpu.restype = C.c_long
        lib.famsa_host_trees_gpu.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, *heur, C.c_char_p, C.c_long,
                                             C.c_void_p, C.c_void_p]
        lib.famsa_host_trees_message.restype = C.c_char_p
        lib.famsa_host_trees_message.argtypes = [C.c_int]
        lib.famsa_host_dist_exports_gpu.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.famsa_host_batch_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p]
        lib.famsa_host_dist_export_gpu.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]
        lib.famsa_host_workset.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        lib.famsa_host_format_distance.argtypes = [C.c_double, C.c_char_p]
        lib.famsa_host_records.restype = C.c_long
        lib.famsa_host_records.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p,
                                           C.c_long]
        lib.famsa_host_clarans.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p]
        lib.famsa_host_newick.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_char_p,
                                          C.c_long]
        lib.famsa_host_newick.restype = C.c_long
        self.lib = lib

    def _err(self):
        return RuntimeError(self.lib.famsa_host_last_error().decode())

    HEUR = {None: 0, "parttree": 1, "medoidtree": 2}

    def _text(self, call, cap=1 << 25):
        """Run a text-returning entry point; -1 = error, <= -2 = the buffer must hold -(n + 1) bytes: retry."""
        for _ in range(2):
            buf = C.create_string_buffer(cap)
            n = call(buf)
            if n >= 0:
                return buf.raw[:n]
            if n == -1:
                raise self._err()
            cap = -(n + 1)
        raise self._err()

    def tree_from_matrix(self, fasta, square, method, distance="indel075_div_lcs", keep_duplicates=False,
                         heuristic=None, subtree_size=0, sample_size=0, threshold=0, cluster_fraction=0.0,
                         cluster_iters=0, num_evals=0, chained_seed=0, dump_seeds=None):
        """`-gt <method> -gt_export` over a caller-supplied oriented LCS matrix; num_evals / chained_seed / dump_seeds are the
        CLI's -num_evals, the seed of -gt chained, and -dump_seeds <file>."""
        sq = np.ascontiguousarray(square, np.uint32)
        return self._text(lambda buf: self.lib.famsa_host_tree_from_matrix_ex(
            fasta.encode(), sq.ctypes.data, method.encode(), DIST[distance], int(keep_duplicates), self.HEUR[heuristic],
            subtree_size, sample_size, threshold, cluster_fraction, cluster_iters, num_evals, chained_seed,
            dump_seeds.encode() if dump_seeds else None, buf, len(buf)))

    def dist_export_from_matrix(self, fasta, square, path, distance="indel075_div_lcs", square_matrix=False,
                                pid=False):
        sq = np.ascontiguousarray(square, np.uint32)
        if self.lib.famsa_host_dist_export_from_matrix(fasta.encode(), sq.ctypes.data, DIST[distance],
                                                       int(square_matrix), int(pid), path.encode()) != 0:
            raise self._err()

    def tree_gpu(self, fasta, method, distance="indel075_div_lcs", keep_duplicates=False, device=0, heuristic=None,
                 subtree_size=0, sample_size=0, threshold=0, cluster_fraction=0.0, cluster_iters=0):
        return self._text(lambda buf: self.lib.famsa_host_tree_gpu(
            fasta.encode(), device, method.encode(), DIST[distance], int(keep_duplicates), self.HEUR[heuristic],
            subtree_size, sample_size, threshold, cluster_fraction, cluster_iters, buf, len(buf)))

    def trees_gpu(self, fastas, method, distance="indel075_div_lcs", keep_duplicates=False, device=0, heuristic=None,
                  subtree_size=0, sample_size=0, threshold=0, cluster_fraction=0.0, cluster_iters=0):
        """Guide trees of many files on one engine context: a list with the Newick bytes of a file or, where the file
        failed, a RuntimeError with its message."""
        n = len(fastas)
        paths = (C.c_char_p * max(n, 1))(*[f.encode() for f in fastas])
        offsets = np.zeros(n + 1, np.int64)
        status = np.zeros(max(n, 1), np.int32)
        cap = 4096
        for f in fastas:
            cap += 64 + (4 * os.path.getsize(f) if os.path.isfile(f) else 0)
        text = self._text(lambda buf: self.lib.famsa_host_trees_gpu(
            C.cast(paths, C.c_void_p), n, device, method.encode(), DIST[distance], int(keep_duplicates), self.HEUR[heuristic],
            subtree_size, sample_size, threshold, cluster_fraction, cluster_iters, buf, len(buf), offsets.ctypes.data,
            status.ctypes.data), cap=cap)
        return [text[int(offsets[i]):int(offsets[i + 1])] if status[i] == 0
                else RuntimeError(self.lib.famsa_host_trees_message(i).decode(errors="replace")) for i in range(n)]

    def batch_plan(self, unique_counts, eligible, pair_budget=0, group_max=0):
        """The batch's chunk planner (no GPU): (chunk number per file, -1 = the one-file route; number of chunks)."""
        counts = np.ascontiguousarray(unique_counts, np.int64)
        flags = np.ascontiguousarray(eligible, np.uint8)
        assert len(counts) == len(flags)
        plan = np.zeros(max(len(counts), 1), np.int32)
        chunks = self.lib.famsa_host_batch_plan(counts.ctypes.data, flags.ctypes.data, len(counts), int(pair_budget), int(group_max),
                                                plan.ctypes.data)
        if chunks < 0:
            raise self._err()
        return plan[: len(counts)].copy(), chunks

    def dist_export_gpu(self, fasta, path, distance="indel075_div_lcs", square_matrix=False, pid=False, device=0):
        if self.lib.famsa_host_dist_export_gpu(fasta.encode(), device, DIST[distance], int(square_matrix), int(pid),
                                               path.encode()) != 0:
            raise self._err()

    def dist_exports_gpu(self, fastas, paths, distance="indel075_div_lcs", square_matrix=False, pid=False, device=0):
        """Distance files of many inputs on one engine context: a list with None for a file made or, where the file
        failed, a RuntimeError with its message."""
        n = len(fastas)
        if len(paths) != n:
            raise ValueError("one output path per input")
        ins = (C.c_char_p * max(n, 1))(*[f.encode() for f in fastas])
        outs = (C.c_char_p * max(n, 1))(*[f.encode() for f in paths])
        status = np.zeros(max(n, 1), np.int32)
        if self.lib.famsa_host_dist_exports_gpu(C.cast(ins, C.c_void_p), C.cast(outs, C.c_void_p), n, device, DIST[distance],
                                                int(square_matrix), int(pid), status.ctypes.data) < 0:
            raise self._err()
        return [None if status[i] == 0 else RuntimeError(self.lib.famsa_host_trees_message(i).decode(errors="replace"))
                for i in range(n)]

    def workset(self, fasta, n, keep_duplicates=False):
        a = np.zeros(n, np.int32)
        b = np.zeros(n, np.int32)
        u = self.lib.famsa_host_workset(fasta.encode(), int(keep_duplicates), a.ctypes.data, b.ctypes.data, n)
        if u < 0:
            raise self._err()
        return u, a, b

    def newick(self, left, right, names, sorted2unique=None):
        """Newick text of the tree whose internal nodes (children left[i], right[i], leaves first) follow the leaves; with
        sorted2unique the duplicates are re-attached first (GuideTree::fromUnique) and names has one entry per record."""
        left = np.ascontiguousarray(left, np.int32)
        right = np.ascontiguousarray(right, np.int32)
        n_leaves = len(left) + 1
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        s2u = None if sorted2unique is None else np.ascontiguousarray(sorted2unique, np.int32)
        cap = 64 + sum(len(n) + 12 for n in names)
        return self._text(lambda buf: self.lib.famsa_host_newick(
            left.ctypes.data, right.ctypes.data, n_leaves, len(left), C.cast(arr, C.c_void_p), len(names),
            None if s2u is None else s2u.ctypes.data, buf, len(buf)), cap=cap)

    def format_distance(self, v):
        buf = C.create_string_buffer(64)
        n = self.lib.famsa_host_format_distance(float(v), buf)
        return buf.raw[:n].decode()

    def clarans(self, triangle, n_elems, n_medoids, n_fixed=1, explore_fraction=0.1, num_local=2):
        tri = np.ascontiguousarray(triangle, np.float32)
        out = np.zeros(n_medoids, np.int32)
        if self.lib.famsa_host_clarans(tri.ctypes.data, n_elems, n_medoids, n_fixed, explore_fraction, num_local,
                                       out.ctypes.data) != 0:
            raise self._err()
        return out

    def records(self, fasta, n_threads=0):
        """(ids, [code arrays]) as the FASTA reader delivers them."""
        size = os.path.getsize(fasta) + 16
        for attempt in range(4):  # a compressed file needs more room than its size on disk
            ids = C.create_string_buffer(size)
            codes = np.zeros(size, np.uint8)
            offs = np.zeros(size // 2 + 2, np.uint64)
            n = self.lib.famsa_host_records(fasta.encode(), n_threads, ids, size, codes.ctypes.data, size,
                                            offs.ctypes.data, len(offs))
            if n >= 0 or b"buffer too small" not in self.lib.famsa_host_last_error():
                break
            size *= 8
        if n < 0:
            raise self._err()
        names = ids.value.decode("latin-1").split("\n")[:-1] if n else []
        return names, [codes[int(offs[i]):int(offs[i + 1])].copy() for i in range(n)]


_HOST = None


def _host():
    global _HOST
    if _HOST is None:
        _HOST = Host()
    return _HOST


def guide_tree(fasta, gt="sl", distance="indel075_div_lcs", keep_duplicates=False, heuristic=None, device=0, **medoid):
    """Newick text (bytes) of `famsa -gt <gt> -gt_export <fasta>`, the LCS and the tree reducers on GPU `device`.
    heuristic: None, "medoidtree" or "parttree" (keyword arguments subtree_size, sample_size, threshold,
    cluster_fraction, cluster_iters as in FAMSA)."""
    return _host().tree_gpu(fasta, gt, distance, keep_duplicates, device, heuristic, **medoid)


def guide_trees(fastas, gt="sl", distance="indel075_div_lcs", keep_duplicates=False, heuristic=None, device=0, on_error="raise",
                **medoid):
    """guide_tree for many files in ONE process on ONE engine context: a list with the Newick text (bytes) of every file, each
    what guide_tree gives for that file alone.  Families up to the routing limit are made together, chunk by chunk (one
    workgroup per family for -gt sl / slink and for upgma / upgma_modified; the host builder over batched triangles for
    nj); the rest goes through the one-file path on the same context.  A file that fails does not stop the others: on_error="raise"
    raises the first failure after all files are done, on_error="return" puts the exception into that file's slot."""
    if on_error not in ("raise", "return"):
        raise ValueError("on_error must be 'raise' or 'return'")
    out = _host().trees_gpu(list(fastas), gt, distance, keep_duplicates, device, heuristic, **medoid)
    if on_error == "raise":
        for r in out:
            if isinstance(r, Exception):
                raise r
    return out


def dist_export(fasta, csv_path, distance="indel075_div_lcs", square_matrix=False, pid=False, device=0):
    """`famsa -dist_export [-square_matrix] [-pid] <fasta> <csv_path>` with the LCS on GPU `device`."""
    _host().dist_export_gpu(fasta, csv_path, distance, square_matrix, pid, device)


def dist_exports(fastas, csv_paths, distance="indel075_div_lcs", square_matrix=False, pid=False, device=0, on_error="raise"):
    """dist_export for many files in ONE process on ONE engine context: csv_paths[i] receives what dist_export writes for
    fastas[i] alone.  Files up to the routing limit are made together, chunk by chunk (one upload and one formatter launch
    sequence per chunk, the files written by worker threads meanwhile); the rest goes through the one-file path on the same
    context.  Returns a list with None per file made.  A file that fails does not stop the others: on_error="raise" raises
    the first failure after all files are done, on_error="return" puts the exception into that file's slot."""
    if on_error not in ("raise", "return"):
        raise ValueError("on_error must be 'raise' or 'return'")
    out = _host().dist_exports_gpu([os.fspath(f) for f in fastas], [os.fspath(f) for f in csv_paths], distance, square_matrix, pid, device)
    if on_error == "raise":
        for r in out:
            if isinstance(r, Exception):
                raise r
    return out
