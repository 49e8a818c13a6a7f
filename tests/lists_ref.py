"""NumPy statement of the complete lists in compressed-sparse-row form (include/acgpt.h: pt_list_offsets, pt_query_overlap_lists,
pt_query_triangles_lists): the CSR arrays of the boolean matrices overlap_ref.overlap_matrix and tritri_ref.intersect_matrix produce,
and the ladder, a scene on which a query's list has any length asked for and is never in ascending order as a walk meets it.  A plain
module shared by tests/test_lists_host.py and tests/test_gpu_lists.py."""
import numpy as np

F = np.float32
NO_PRIM = np.uint32(0xFFFFFFFF)
LENGTH_CLASSES = ((0, 0), (1, 8), (9, 64), (65, 256), (257, None))      # list lengths: none, the capped calls' 8, and beyond


def offsets_of(counts):
    """uint64 [n + 1]: 0 and the running sums of the counts"""
    out = np.zeros(len(counts) + 1, np.uint64)
    np.cumsum(np.asarray(counts, np.uint64), out=out[1:])
    return out


def csr_of_matrix(m):
    """(offsets uint64 [n + 1], prims uint32 [total], counts uint32 [n]) of a bool [n, n_tris] matrix: row i's true columns ascending in
    prims[offsets[i]:offsets[i + 1]]"""
    m = np.asarray(m, bool)
    counts = m.sum(axis=1).astype(np.uint32)
    prims = np.nonzero(m)[1].astype(np.uint32)          # row-major: ascending within a row
    return offsets_of(counts), prims, counts


def class_shares(counts):
    """per LENGTH_CLASSES entry the number of queries whose list length falls in it"""
    c = np.asarray(counts, np.int64)
    return tuple(int((c >= lo).sum() if hi is None else ((c >= lo) & (c <= hi)).sum()) for lo, hi in LENGTH_CLASSES)


# ---- the ladder ----------------------------------------------------------------------------------------------------------------------
LADDER_T = 20000
LADDER_SEED = 20241


def ladder_perm(T=LADDER_T, seed=LADDER_SEED):
    """perm[p]: the index of the triangle at position x = p.  A fixed-seed permutation whose first two entries descend, so that even
    the list of length 2 is not ascending in position order."""
    perm = np.random.default_rng(seed).permutation(T).astype(np.uint32)
    if T >= 2 and perm[0] < perm[1]:
        perm[[0, 1]] = perm[[1, 0]]
    return perm


def ladder(T=LADDER_T, seed=LADDER_SEED):
    """(verts [3 T, 4] f32, idx [T, 3] u32): T small disjoint triangles in the plane z = 0, the one at position p being
    {(p - 0.2, 0), (p + 0.2, 0), (p, 0.2)} and having index perm[p].  The box [-0.5, k - 0.5] in x overlaps exactly the k triangles at
    positions 0 .. k - 1, whose indices perm[:k] are unrelated to any order a walk along x, or through a tree built over x, meets."""
    perm = ladder_perm(T, seed)
    pos = np.empty(T, np.int64)
    pos[perm] = np.arange(T)                             # pos[j]: where triangle j sits
    p = pos.astype(np.float32)
    v = np.zeros((T, 3, 4), np.float32)
    v[:, 0, 0], v[:, 1, 0], v[:, 2, 0] = p - F(0.2), p + F(0.2), p
    v[:, 2, 1] = F(0.2)
    return v.reshape(-1, 4), np.arange(3 * T, dtype=np.uint32).reshape(-1, 3)


def ladder_boxes(lengths):
    """(n, 8) box records: box i spans [-0.5, lengths[i] - 0.5] in x (centre and half extent exact in fp32) and the triangles' y and z"""
    k = np.asarray(lengths, np.float32)
    b = np.zeros((k.size, 8), np.float32)
    b[:, 0], b[:, 3] = k * F(0.5) - F(0.5), k * F(0.5)
    b[:, 1], b[:, 4], b[:, 5] = F(0.05), F(1.0), F(1.0)
    return b


def ladder_triangles(lengths):
    """(n, 12) query triangles, long and thin along x: {(-0.5, 0.05, 0), (k - 0.5, 0.05, 0), (k - 0.5, 0.05, 1)}.  The first edge lies in
    the triangles' plane and runs through the inside of those at positions 0 .. k - 1; length 0 is a point at x = -0.5."""
    k = np.asarray(lengths, np.float32)
    r = np.zeros((k.size, 3, 4), np.float32)
    r[:, 0, 0], r[:, 1, 0], r[:, 2, 0] = F(-0.5), k - F(0.5), k - F(0.5)
    r[:, :, 1] = F(0.05)
    r[:, 2, 2] = F(1.0)
    return r.reshape(-1, 12)


def ladder_expected(lengths, T=LADDER_T, seed=LADDER_SEED):
    """(offsets, prims, counts) the ladder's construction promises: list i is perm[:lengths[i]] sorted"""
    perm = ladder_perm(T, seed)
    counts = np.asarray(lengths, np.uint32)
    prims = np.concatenate([np.sort(perm[:k]) for k in counts] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return offsets_of(counts), prims, counts
