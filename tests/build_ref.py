"""Sequential statements of the three stages behind build modes 1 and 2 of csrc/lbvh_build.hip, each from its algorithm: PLOC (numpy,
float32), the host insertion pass (plain Python, float32 scalars) and the parallel reinsertion of the device (C++: oracle/build_ref.cpp,
loaded with ctypes).  tests/test_gpu_build_ref.py holds the device's trees to them word for word; tests/test_build_ref_host.py holds
the statements themselves to slower ones and shows that the test scenes depend on every rule.  No GPU.

A tree is the fp32 node array as pt_debug_read_tree(1) gives it: uint32 [m, 16] per inner node = child 0's box lo xyz, hi xyz, child 1's
box lo xyz, hi xyz, the two child references (>= 0 inner node, ~slot leaf), two zero words; node 0 is the root.  Every stage takes leaf
boxes or such an array and returns such an array, so the stages chain.

PLOC (ploc)   Clusters in Morton order, each a box, a reference and a height.  Per round every cluster looks RADIUS positions to each
    side for the partner with the smallest merged area dx*dy + dy*dz + dz*dx (float32, as written); ties go to the lower position, or —
    once `hashed` — to the pair whose lower position i has the smaller i * 0x9E3779B1 mod 2^32.  Two clusters that chose each other
    merge: the node (lower, upper) takes the next number DOWNWARDS from n - 2, numbers handed out in position order within a round; the
    merged cluster stays at the lower position, the sequence closes up.  Rounds run in batches of eight; after a batch that began with
    more than 1024 clusters and took less than a quarter off, `hashed` is set for good.
Host insertion pass (insertion_pass)   lbvh_build.hip section 12: per pass the inner nodes but the root in descending area, ties by
    number; a node whose parent is the root stays; otherwise node and parent leave the tree (the sibling moves up, boxes refitted until
    one does not change), and the node's two subtrees, the larger first, go back in where a best-first search over (induced area,
    reference) finds the least added area, reusing the two free node numbers; the root keeps number 0.  Passes until one leaves
    more than 0.995 of the area sum (float64 sum of float32 areas in node order), eight at most.
Device reinsertion (reinsert)   see oracle/build_ref.cpp.

ALTER names the test-only switches: each changes one rule, for the sensitivity test."""
import ctypes as C
import heapq
import os
import subprocess

import numpy as np

import tree_ref as tr

F = np.float32
RADIUS = 8
BATCH = 8
K_OPTIMIZE_MAX_TRIS = tr.K_OPTIMIZE_MAX_TRIS
K_REINSERT_ITERATIONS = 12
ORACLE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")

ALTER = ("radius7", "ties_high", "upper_keeps", "no_hash", "ascending_area", "smaller_first", "no_through_locks", "key_node_first", "no_sibling_exclusion")
_RI_BITS = {"no_through_locks": 1, "key_node_first": 2, "no_sibling_exclusion": 4}


# ---- the leaves: records in Morton order -------------------------------------------------------------------------------------------

def _expand10(v):
    v = (v * np.uint32(0x00010001)) & np.uint32(0xFF0000FF)
    v = (v * np.uint32(0x00000101)) & np.uint32(0x0F00F00F)
    v = (v * np.uint32(0x00000011)) & np.uint32(0xC30C30C3)
    return (v * np.uint32(0x00000005)) & np.uint32(0x49249249)


def morton_order(verts, idx):
    """(codes sorted, prims sorted): the 30-bit codes of the triangle boxes' centres in the scene box, sorted, equal codes by triangle
    number (the CPU tests' stand-in for pt_read_morton; the GPU tests take the device's order and hold this one to it)"""
    n = len(idx)
    tw = tr.records_of(verts, idx, np.zeros(n, np.uint32), np.arange(n))
    lo, hi = tr.record_boxes(tw, tr.pad_abs_of(verts))
    slo, shi = lo.min(axis=0), hi.max(axis=0)
    c = (F(0.5) * (lo + hi).astype(F)).astype(F)
    ext = (shi - slo).astype(F)
    with np.errstate(all="ignore"):
        u = np.where(ext > 0, ((c - slo).astype(F) / ext).astype(F), F(0.0))
    q = np.minimum(np.maximum((u * F(1024.0)).astype(F), F(0.0)), F(1023.0)).astype(np.uint32)
    codes = (_expand10(q[:, 0]) << np.uint32(2)) | (_expand10(q[:, 1]) << np.uint32(1)) | _expand10(q[:, 2])
    order = np.argsort(codes, kind="stable")
    return codes[order], order.astype(np.uint32)


def leaf_boxes(verts, idx, prims=None):
    """(lo, hi) float32 [n, 3] of the triangles in slot order (prims: pt_read_morton's, or this module's Morton order)"""
    if prims is None:
        prims = morton_order(verts, idx)[1]
    tw = tr.records_of(verts, idx, np.zeros(len(idx), np.uint32), prims)
    return tr.record_boxes(tw, tr.pad_abs_of(verts))


# ---- the node layout ---------------------------------------------------------------------------------------------------------------

def split(nodes):
    """(children int32 [m, 2], lo [m, 2, 3], hi [m, 2, 3]) of an fp32 node array"""
    w = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
    lo, hi = tr.fp32_boxes(w)
    return tr.children_of(1, w)[0], lo, hi


def height_of(nodes):
    """inner nodes on the longest root-to-leaf path"""
    ch = split(nodes)[0]
    depth, level = 0, np.array([0], np.int64)
    while level.size:
        assert depth <= len(ch)
        depth += 1
        c = ch[level].reshape(-1)
        level = c[c >= 0].astype(np.int64)
    return depth


def area_sum(nodes):
    """float64 sum, in node order, of the float32 surface measures x*y + y*z + z*x of the inner nodes' boxes"""
    _, lo, hi = split(nodes)
    d = (hi.max(axis=1) - lo.min(axis=1)).astype(F)
    a = ((d[:, 0] * d[:, 1]).astype(F) + (d[:, 1] * d[:, 2]).astype(F)).astype(F) + (d[:, 2] * d[:, 0]).astype(F)
    s = 0.0
    for x in a.astype(F).tolist():
        s += x
    return s


def depth_first(nodes):
    """the same tree with its inner nodes numbered in pre-order (what build_impl does above kDepthFirstTris triangles): a node, then the
    subtree of its first child, then that of its second"""
    w = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
    ch = tr.children_of(1, w)[0].tolist()
    new, stack, count = [0] * len(ch), [0], 0
    while stack:
        i = stack.pop()
        new[i] = count
        count += 1
        stack += [c for c in (ch[i][1], ch[i][0]) if c >= 0]
    new = np.array(new)
    out = np.zeros_like(w)
    out[new] = w
    c = out[:, 12:14].view(np.int32)
    out[:, 12:14] = np.where(c >= 0, new[np.maximum(c, 0)], c).astype(np.int32).view(np.uint32)
    return out


# ---- PLOC --------------------------------------------------------------------------------------------------------------------------

def _merged_area(lo_a, hi_a, lo_b, hi_b):
    d = (np.maximum(hi_a, hi_b) - np.minimum(lo_a, lo_b)).astype(F)
    return (((d[..., 0] * d[..., 1]).astype(F) + (d[..., 1] * d[..., 2]).astype(F)).astype(F) + (d[..., 2] * d[..., 0]).astype(F)).astype(F)


def nearest_partners(lo, hi, hashed, radius=RADIUS, ties_high=False):
    """per position the chosen partner's position (the position itself where it has none)"""
    m = len(lo)
    pos = np.arange(m)
    offs = np.array([d for d in range(-radius, radius + 1) if d != 0])
    j = pos[:, None] + offs[None, :]
    ok = (j >= 0) & (j < m)
    jc = np.clip(j, 0, m - 1)
    ar = np.where(ok, _merged_area(lo[:, None, :], hi[:, None, :], lo[jc], hi[jc]), F(np.inf))
    assert np.isfinite(ar[ok]).all()
    cand = ok & (ar == ar.min(axis=1, keepdims=True))
    if hashed:
        key = (np.minimum(pos[:, None], jc).astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
        key = np.where(cand, key, np.uint64(1 << 32))
        cand &= key == key.min(axis=1, keepdims=True)
    pick = (cand.shape[1] - 1 - np.argmax(cand[:, ::-1], axis=1)) if ties_high else np.argmax(cand, axis=1)
    return np.where(cand.any(axis=1), jc[pos, pick], pos)


def ploc(leaf_lo, leaf_hi, alter=None, partners=nearest_partners):
    """(nodes uint32 [n - 1, 16], rounds, root height, hashed: whether ties went to hashed pairs at some point)"""
    n = len(leaf_lo)
    assert n >= 2
    lo, hi = np.array(leaf_lo, F), np.array(leaf_hi, F)
    ref = ~np.arange(n, dtype=np.int32)
    height = np.zeros(n, np.int64)
    nodes = np.zeros((n - 1, 16), np.uint32)
    fv = nodes.view(F)
    next_top, rounds, hashed = n - 2, 0, False
    radius = 7 if alter == "radius7" else RADIUS
    while len(lo) > 1:
        before = len(lo)
        for _ in range(BATCH):
            m = len(lo)
            if m < 2:
                break
            nn = partners(lo, hi, hashed, radius, alter == "ties_high")
            pos = np.arange(m)
            mutual = (nn != pos) & (nn[nn] == pos)
            low = np.flatnonzero(mutual & (pos < nn))            # the lower partner of every pair, in position order
            up = nn[low]
            assert low.size, "no mutual pair"
            number = next_top - np.arange(low.size)
            fv[number, 0:3], fv[number, 3:6], fv[number, 6:9], fv[number, 9:12] = lo[low], hi[low], lo[up], hi[up]
            nodes[number, 12], nodes[number, 13] = ref[low].view(np.uint32), ref[up].view(np.uint32)
            stay = up if alter == "upper_keeps" else low
            lo[stay], hi[stay] = np.minimum(lo[low], lo[up]), np.maximum(hi[low], hi[up])
            height[stay] = 1 + np.maximum(height[low], height[up])
            ref[stay] = number.astype(np.int32)
            keep = np.ones(m, bool)
            keep[low if alter == "upper_keeps" else up] = False
            lo, hi, ref, height = lo[keep], hi[keep], ref[keep], height[keep]
            next_top -= low.size
            rounds += 1
        if not hashed and alter != "no_hash" and before > 1024 and len(lo) > before - before // 4:
            hashed = True
    assert next_top == -1 and ref[0] == 0
    return nodes, rounds, int(height[0]), hashed


def partners_by_definition(lo, hi, hashed, radius=RADIUS, ties_high=False):
    """nearest_partners again, one pair at a time: the table of merged areas, then the smallest entry by (area, hash, position)"""
    m = len(lo)
    out = np.arange(m)
    for i in range(m):
        best = None
        for j in range(max(0, i - radius), min(m, i + radius + 1)):
            if j == i:
                continue
            d = [F(max(hi[i][k], hi[j][k])) - F(min(lo[i][k], lo[j][k])) for k in range(3)]
            a = F(F(d[0] * d[1]) + F(d[1] * d[2])) + F(d[2] * d[0])
            key = (float(a), (min(i, j) * 0x9E3779B1) & 0xFFFFFFFF if hashed else 0, j)
            if best is None or key < best:
                best = key
        if best is not None:
            out[i] = best[2]
    return out


# ---- the host insertion pass -------------------------------------------------------------------------------------------------------

def _area(b):
    x, y, z = b[3] - b[0], b[4] - b[1], b[5] - b[2]
    return x * y + y * z + z * x


def _union(a, b):
    return (min(a[0], b[0]), min(a[1], b[1]), min(a[2], b[2]), max(a[3], b[3]), max(a[4], b[4]), max(a[5], b[5]))


class _HostTree:
    """inner nodes 0 .. m-1, leaves ~slot; boxes as 6-tuples of numpy float32 scalars (every operation on them rounds to float32)"""

    def __init__(self, nodes):
        ch, lo, hi = split(nodes)
        self.m = m = len(ch)
        self.child = [[int(ch[i, 0]), int(ch[i, 1])] for i in range(m)]
        self.nbox, self.nparent = [None] * m, [-1] * m
        self.lbox, self.lparent = [None] * (m + 1), [-1] * (m + 1)
        for i in range(m):
            for k in (0, 1):
                b = tuple(lo[i, k]) + tuple(hi[i, k])
                c = self.child[i][k]
                if c >= 0:
                    self.nbox[c], self.nparent[c] = b, i
                else:
                    self.lbox[~c], self.lparent[~c] = b, i
        self.nbox[0] = _union(self.box(self.child[0][0]), self.box(self.child[0][1]))

    def box(self, r):
        return self.nbox[r] if r >= 0 else self.lbox[~r]

    def set_parent(self, r, p):
        if r >= 0:
            self.nparent[r] = p
        else:
            self.lparent[~r] = p

    def parent(self, r):
        return self.nparent[r] if r >= 0 else self.lparent[~r]

    def replace_child(self, p, old, new):
        self.child[p][0 if self.child[p][0] == old else 1] = new

    def refit_from(self, node):
        while node >= 0:
            b = _union(self.box(self.child[node][0]), self.box(self.child[node][1]))
            if b == self.nbox[node]:
                return
            self.nbox[node] = b
            node = self.nparent[node]

    def area_sum(self):
        s = 0.0
        for b in self.nbox:
            s += float(_area(b))
        return s

    def find_insertion(self, b):
        """the reference next to which a subtree with box b adds least area: best first over (area added above, reference)"""
        ab = _area(b)
        best, best_ref = F(np.inf), 0
        heap = [(F(0.0), 0)]
        while heap:
            induced, r = heapq.heappop(heap)
            if induced + ab >= best:
                break
            total = induced + _area(_union(self.box(r), b))
            if total < best:
                best, best_ref = total, r
            if r >= 0:
                below = total - _area(self.nbox[r])
                if below + ab < best:
                    heapq.heappush(heap, (below, self.child[r][0]))
                    heapq.heappush(heap, (below, self.child[r][1]))
        return best_ref

    def insert_at(self, at, sub, q):
        """the free node q takes the place of `at` and holds (at, sub); at the root, q takes the root's content instead"""
        if at == 0:
            self.child[q] = list(self.child[0])
            for c in self.child[q]:
                self.set_parent(c, q)
            self.nbox[q] = self.nbox[0]
            self.child[0] = [q, sub]
            self.nparent[q] = 0
            self.set_parent(sub, 0)
            self.nbox[0] = _union(self.nbox[q], self.box(sub))
            return
        p = self.parent(at)
        self.replace_child(p, at, q)
        self.nparent[q] = p
        self.child[q] = [at, sub]
        self.set_parent(at, q)
        self.set_parent(sub, q)
        self.nbox[q] = _union(self.box(at), self.box(sub))
        self.refit_from(p)

    def one_pass(self, alter=None):
        order = sorted(range(1, self.m), key=lambda i: ((1 if alter == "ascending_area" else -1) * float(_area(self.nbox[i])), i))
        for x in order:
            p = self.nparent[x]
            if p <= 0:
                continue
            g = self.nparent[p]
            sib = self.child[p][1 if self.child[p][0] == x else 0]
            l, r = self.child[x]
            self.replace_child(g, p, sib)
            self.set_parent(sib, g)
            self.refit_from(g)
            l_first = _area(self.box(l)) >= _area(self.box(r))
            if alter == "smaller_first":
                l_first = not l_first
            first, second = (l, r) if l_first else (r, l)
            self.insert_at(self.find_insertion(self.box(first)), first, p)
            self.insert_at(self.find_insertion(self.box(second)), second, x)

    def nodes(self):
        out = np.zeros((self.m, 16), np.uint32)
        f = out.view(F)
        for i in range(self.m):
            for k in (0, 1):
                f[i, 6 * k:6 * k + 6] = self.box(self.child[i][k])
                out[i, 12 + k] = np.int32(self.child[i][k]).view(np.uint32)
        return out


def insertion_pass(nodes, max_passes=8, stop=0.995, alter=None):
    """(nodes, passes, area sum before, area sum after — float64)"""
    t = _HostTree(nodes)
    before = prev = t.area_sum()
    done = 0
    while done < max_passes:
        t.one_pass(alter)
        done += 1
        now = t.area_sum()
        if not now < prev * stop:
            break
        prev = now
    return t.nodes(), done, before, t.area_sum()


# ---- the device's parallel reinsertion ---------------------------------------------------------------------------------------------

_lib = None


def _library():
    global _lib
    if _lib is None:
        path = os.path.join(ORACLE_DIR, "libbuild_ref.so")
        src = os.path.join(ORACLE_DIR, "build_ref.cpp")
        if not os.path.exists(path) or os.path.getmtime(src) > os.path.getmtime(path):
            subprocess.run(["make", "-C", ORACLE_DIR, "libbuild_ref.so"], check=True, stdout=subprocess.DEVNULL)
        _lib = C.CDLL(path)
        vp, u = C.c_void_p, C.c_uint32
        _lib.bref_find.argtypes = [vp, u, u, u, vp, vp, vp, vp]
        _lib.bref_find.restype = C.c_int
        _lib.bref_reinsert.argtypes = [vp, u, u, u, u, vp, vp, vp, vp, vp]
        _lib.bref_reinsert.restype = C.c_int
    return _lib


class Reinserted:
    """nodes[r]: the tree after round r + 1; winners[r]; area[r], height[r]: after r rounds (0: the tree as given); caps: the most pivots,
    search steps and through-path nodes any move needed; shared: pairs of winners of one round with a common edited node; broken: the
    round after which the references were no tree (0: never)"""


def reinsert(nodes, rounds=K_REINSERT_ITERATIONS, alter=None):
    w = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
    m = len(w)
    out = Reinserted()
    trees = np.zeros((rounds, m, 16), np.uint32)
    winners, height, checks = np.zeros(rounds, np.uint32), np.zeros(rounds + 1, np.uint32), np.zeros(5, np.uint32)
    area = np.zeros(rounds + 1, np.float64)
    done = _library().bref_reinsert(w.ctypes.data, m, m + 1, rounds, _RI_BITS.get(alter, 0), trees.ctypes.data, winners.ctypes.data, area.ctypes.data,
                                    height.ctypes.data, checks.ctypes.data)
    out.nodes, out.winners, out.area, out.height = trees[:done], winners[:done], area[:done + 1], height[:done + 1]
    out.caps, out.shared, out.broken = tuple(int(x) for x in checks[:3]), int(checks[3]), int(checks[4])
    return out


def rounds_by_stop_rule(r, max_rounds=K_REINSERT_ITERATIONS, stop=0.998):
    """how many rounds the build's stop rule runs on the reference's own sums: it ends with the first round that has no winners or does
    not bring the sum below `stop` of the sum before it"""
    for k in range(min(max_rounds, len(r.winners))):
        if r.winners[k] == 0 or not r.area[k + 1] < r.area[k] * stop:
            return k + 1
    return min(max_rounds, len(r.winners))


def best_moves(nodes, alter=None):
    """(target, pivot, gain float32, caps) per unified node number (inner nodes 0 .. m-1, leaf slot s = m + s; -1: no move)"""
    w = np.ascontiguousarray(nodes, np.uint32).reshape(-1, 16)
    m = len(w)
    target, pivot, gain, caps = np.zeros(2 * m + 1, np.int32), np.zeros(2 * m + 1, np.int32), np.zeros(2 * m + 1, F), np.zeros(3, np.uint32)
    assert _library().bref_find(w.ctypes.data, m, m + 1, _RI_BITS.get(alter, 0), target.ctypes.data, pivot.ctypes.data, gain.ctypes.data, caps.ctypes.data) == 0
    return target, pivot, gain, caps


# ---- a whole build -----------------------------------------------------------------------------------------------------------------

def build(leaf_lo, leaf_hi, mode, alter=None, max_passes=8, max_rounds=K_REINSERT_ITERATIONS):
    """What build_impl does after the sort, for modes 1 and 2: dict(nodes, rounds, height, hashed, ploc; mode 2 also passes, before,
    after and — above kOptimizeMaxTris — the Reinserted record `ri`)"""
    n = len(leaf_lo)
    nodes, rounds, height, hashed = ploc(leaf_lo, leaf_hi, alter)
    out = dict(nodes=nodes, ploc=nodes, rounds=rounds, height=height, hashed=hashed, passes=0)
    if mode == 2 and 2 < n <= K_OPTIMIZE_MAX_TRIS:
        out["nodes"], out["passes"], out["before"], out["after"] = insertion_pass(nodes, max_passes, alter=alter)
        out["height"] = height_of(out["nodes"])
    elif mode == 2 and n > K_OPTIMIZE_MAX_TRIS:
        ri = reinsert(nodes, max_rounds, alter)
        k = rounds_by_stop_rule(ri, max_rounds)
        out.update(ri=ri, passes=k, before=ri.area[0], after=ri.area[k], nodes=ri.nodes[k - 1] if k else nodes, height=int(ri.height[k]))
    return out
