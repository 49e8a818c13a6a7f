"""The validator of a built BVH as the device holds it (pt_debug_read_tree, include/acgpt_test.h): every node, child and plane of every
array, against the triangles.  Plain numpy: float32 where the device's single operations are reproduced (every one is one correctly
rounded operation or a min / max, so the bits follow), float64 elsewhere.  No GPU, no library.

validate(arrays, info, verts, idx, mat_ids, ...) takes the raw arrays as uint32 words ({what: words}, `what` as pt_debug_read_tree
numbers them: 1 fp32 nodes, 2 fp16 {lo, hi} nodes, 3 fp16 {centre, half extent} nodes, 4 four-wide records, 5 triangle records, 6 shade
records), the info struct (any object with pt_tree_info's fields) and the scene as the caller passed it.  It returns a list of
Violation(check, array, node, child, axis, values); an empty list is a valid tree.  Per (check, array) the first `cap` violations are
listed and one more entry (node -1) carries the total, but every node is checked.  The list's .slack maps an array to the largest
distance between a stored plane and the exact one, as a share of the bound below (information, no verdict).

Triangle records (5, 6)   prim words a permutation of 0 .. n-1 in pt_read_morton's order; v0, e1 = b - a, e2 = c - a the fp32
    subtractions of the caller's vertices bit for bit; material word (low 24 bits) = mat_ids[prim] in both records; shade normal within
    4 ulp per component of float64 normalize(cross(e1, e2)) — plus what the cross product's own fp32 roundings do to it, which no fp32
    evaluation avoids where the two products of a component cancel: err_j = 2^-24 (|e1_k e2_l| + |e1_l e2_k| + |cross_j|) per component
    (two products and a difference, half an ulp each), felt by n_i directly and through the length:
    (err_i + |n_i| sum_j |n_j| err_j) / |cross|.  The 4 ulp are the normalisation's: dot, sqrt, reciprocal, product.
    Zero-area triangles are left out of the normal check only.
Topology   n_nodes = max(n_tris - 1, 1); node 0 nobody's child, every other inner index and every leaf slot (~slot) referenced exactly
    once, everything reachable from node 0; the longest root-to-leaf path in inner nodes EQUALS max_depth and is at most
    stack_entries - 1; every node array carries the same child references (inner ones shifted by 5 in the centre / half-extent nodes).
    The only empty child box accepted is the second child of the one node of a one-triangle scene (which references slot 0 again).
fp32 boxes (1)   each child box = the fp32 min / max union of record_aabb over the records below it, bit for bit (unions are exact);
    record_aabb: corners v0, v0 + e1, v0 + e2, pad = max(1e-5f * max(1, |l|, |h|), pad_abs); pad_abs = coord_max / 524288 over every
    finite vertex coordinate, at least 2^-19; the root's union = scene_lo / scene_hi; HSpace = build_impl's fp32 expressions.
fp16 {lo, hi} nodes (2)   g the decoded half, a = (w - c) / inv_scale in float64 of the exact fp32 plane w:
    containment  g_lo <= a_lo - |a_lo| 2^-19, g_hi >= a_hi + |a_hi| 2^-19      tightness  |g - a| <= ulp16(g) + |a| 2^-17
    From pack_planes: a' = (w - c) * (1 / inv_scale) carries three fp32 roundings (3 x 2^-24 |a| = 1.8e-7 |a|), the guard moves it
    outward by 3.9e-6 |a'| (one more rounding, 6e-8 |a|), then ONE outward fp16 rounding (< ulp16 of the result).  Outward by at least
    (3.9 - 0.25)e-6 |a| > 2^-19 |a| = 1.9e-6 |a|; by at most (3.9 + 0.25)e-6 |a| + ulp16(g) < 2^-17 |a| + ulp16(g).
fp16 {centre, half extent} nodes (3)   per-axis scales isx / isy / isz, m = max(|a_lo|, |a_hi|):
    containment  c - h <= a_lo - m 2^-19, c + h >= a_hi + m 2^-19
    tightness    h <= (a_hi - a_lo) / 2 + ulp16(c) / 2 + m 2^-17 + ulp16(h)
    centre       |c - (a_lo + a_hi) / 2| <= ulp16(c) / 2 + m 2^-21   (round to nearest of an fp32 midpoint that is within 2^-22 m of
                 the exact one: three roundings per end, one for the sum)
    From pack_centre_half: h' = max(b - c, c - a) + 3.9e-6 m = (b - a) / 2 + |c - mid| + 3.9e-6 m, times (1 + 1e-6) (h' <= m), plus
    fp32 roundings (< 0.4e-6 m), one upward fp16 rounding: at most 5.3e-6 m < 2^-17 m beyond (b - a) / 2 + ulp16(c) / 2, + ulp16(h).
    Empty child: h < 0.  Inner child words are index << 5 exactly.
Four-wide records (4)   plane = origin + 2^(e - 127) * byte in float64.  Children of a wide node are consecutive records from `base`,
    inner nodes first, n_children in 1 .. 4, n_inner in 0 .. n_children (a node above triangles only has no inner child); every record
    is reached once, every triangle record's 48 bytes equal the TriRecord of its slot, every slot appears once; the triangles below a
    child are those below ONE node or leaf of the two-child tree; the decoded box contains that subtree's fp32 box by at least margin =
    kMarginRel (2^-20) x max(1, largest |scene_lo / hi| component, largest extent) and exceeds it by at most one cell 2^(e - 127)
    plus twice the margin (encode(): floor / ceil of the plane moved out by one margin; the origin is the fp32 at or below the lowest
    such plane, less than a margin below it).  Exponent rule, read off encode(): e starts at max(ceil(log2(ext / 255)), -100), ext =
    (highest hi + margin) - origin, and grows while a child's hi byte would pass 255; so e is the smallest exponent with
    255 * 2^e >= ext (or -100): checked as 255 * 2^e >= ext and, for e > -100, 255 * 2^(e - 1) < ext.  Unused slots hold lo byte 255,
    hi byte 0.  The number of levels = wide_depth, the number of wide nodes = n_wnodes, n_wrecs = n_wnodes + n_tris.
Karras trees (build mode 0)   the leaves under every inner node are a contiguous slot range, and the set of ranges is the set
    radix_tree() gives over the keys code << 32 | slot (k_hierarchy's tie rule: delta = 32 + clz(i ^ j) for equal codes, i.e. the
    common prefix of the 64-bit keys).  Sets of ranges, not node numbers: above kDepthFirstTris the nodes are renumbered.
Depth-first numbering (depth_first=True; scenes above kDepthFirstTris)   an inner first child is its parent + 1, an inner second child
    its parent + 1 + the inner nodes below the first child."""
import numpy as np

F = np.float32
K_DEPTH_FIRST_TRIS = 50000
K_OPTIMIZE_MAX_TRIS = 16384
K_MARGIN_REL = 2.0 ** -20
NAMES = {0: "info", 1: "fp32", 2: "h16", 3: "hc16", 4: "wide", 5: "tris", 6: "shade"}


class Info:
    """pt_tree_info as plain Python values"""
    FIELDS = ("n_tris", "n_nodes", "max_depth", "mode", "pad_abs", "hspace", "scene_lo", "scene_hi", "n_wrecs", "n_wnodes", "wide_depth", "held")

    def __init__(self, **kw):
        for k in self.FIELDS:
            setattr(self, k, kw.get(k, 0))

    @classmethod
    def of(cls, s):
        """from the ctypes struct (arrays become float32 numpy arrays)"""
        o = cls()
        for k in cls.FIELDS:
            v = getattr(s, k)
            setattr(o, k, np.array(list(v), F) if hasattr(v, "__len__") else (F(v) if k == "pad_abs" else int(v)))
        return o


class Violation:
    def __init__(self, check, array, node, child=-1, axis=-1, values=None):
        self.check, self.array, self.node, self.child, self.axis, self.values = check, array, int(node), int(child), int(axis), values

    def __repr__(self):
        return "%s[%s] node %d child %d axis %d: %s" % (self.check, self.array, self.node, self.child, self.axis, self.values)


class Violations(list):
    def __init__(self, cap=12):
        super().__init__()
        self.cap, self.totals, self.slack = cap, {}, {}

    def add(self, check, array, node, child=-1, axis=-1, values=None):
        k = (check, array)
        self.totals[k] = self.totals.get(k, 0) + 1
        if self.totals[k] <= self.cap:
            self.append(Violation(check, array, node, child, axis, values))

    def add_where(self, check, array, mask, nodes, values):
        """mask [m, 2 or 4, 3] or [m, 2] or [m]: one violation per set entry; nodes [m]: node numbers; values(i, ...) -> text"""
        mask = np.asarray(mask)
        total = int(mask.sum())
        if total == 0:
            return
        k = (check, array)
        room = max(self.cap - self.totals.get(k, 0), 0)
        for pos in np.argwhere(mask)[:room]:
            pos = tuple(int(p) for p in pos)
            self.add(check, array, nodes[pos[0]], pos[1] if len(pos) > 1 else -1, pos[2] if len(pos) > 2 else -1, values(*pos))
        self.totals[k] = self.totals.get(k, 0) + total - min(room, total)

    def finish(self):
        for (check, array), n in self.totals.items():
            if n > self.cap:
                self.append(Violation(check, array, -1, values="%d violations in all, %d listed" % (n, self.cap)))
        return self

    def note_slack(self, array, share):
        if share.size:
            self.slack[array] = max(self.slack.get(array, 0.0), float(np.max(share)))


# ---- number formats ----------------------------------------------------------------------------------------------------------------

def ulp16(g):
    """spacing of fp16 at |g| (float64 in, float64 out)"""
    return np.spacing(np.abs(np.asarray(g, np.float64)).astype(np.float16)).astype(np.float64)


def halves(w):
    """(low half, high half) of packed words as float64"""
    w = np.ascontiguousarray(w, np.uint32)
    lo = (w & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float64)
    hi = (w >> 16).astype(np.uint16).view(np.float16).astype(np.float64)
    return lo, hi


def half_rd(x):
    """__float2half_rd of float32 x: the bits (uint16)"""
    x = np.asarray(x, F)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    over = h.astype(F) > x
    h[over] = np.nextafter(h[over], np.float16(-np.inf))
    return h.view(np.uint16)


def half_ru(x):
    x = np.asarray(x, F)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    under = h.astype(F) < x
    h[under] = np.nextafter(h[under], np.float16(np.inf))
    return h.view(np.uint16)


def pack_planes(lo, hi, c, inv_scale):
    """pt_device.h pack_planes in float32: packed words (uint32) of fp32 intervals [lo, hi] (arrays), centre c, HSpace.inv_scale"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    scale = F(1.0) / F(inv_scale)
    with np.errstate(invalid="ignore"):
        a, b = ((lo - F(c)).astype(F) * scale).astype(F), ((hi - F(c)).astype(F) * scale).astype(F)
        hl = half_rd(a - np.abs(a) * F(3.9e-6))
        hh = half_ru(b + np.abs(b) * F(3.9e-6))
    out = hl.astype(np.uint32) | (hh.astype(np.uint32) << 16)
    return np.where(lo <= hi, out, np.uint32(0x7C00 | (0xFC00 << 16))).astype(np.uint32)


def pack_centre_half(lo, hi, c0, inv_scale):
    """pt_device.h pack_centre_half in float32 (inv_scale: the axis' HSpace.is*)"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    scale = F(1.0) / F(inv_scale)
    with np.errstate(invalid="ignore"):
        a, b = ((lo - F(c0)).astype(F) * scale).astype(F), ((hi - F(c0)).astype(F) * scale).astype(F)
        hc = (F(0.5) * a + F(0.5) * b).astype(F).astype(np.float16)
        c = hc.astype(F)
        guard = np.maximum(np.abs(a), np.abs(b)) * F(3.9e-6)
        h = np.maximum(b - c, c - a) + guard
        hh = half_ru(h + np.abs(h) * F(1e-6))
    out = hc.view(np.uint16).astype(np.uint32) | (hh.astype(np.uint32) << 16)
    empty = np.uint32(int(np.float16(0.0).view(np.uint16)) | (int(np.float16(-1.0).view(np.uint16)) << 16))
    return np.where(lo <= hi, out, empty).astype(np.uint32)


def pad_abs_of(verts):
    xyz = np.abs(np.asarray(verts, F).reshape(len(verts), -1)[:, :3]).reshape(-1)
    xyz = xyz[np.isfinite(xyz)]
    m = max(F(1.0), xyz.max()) if xyz.size else F(1.0)
    return F(F(m) * F(1.0 / 524288.0))


def hspace_of(scene_lo, scene_hi):
    """The eight HSpace floats of build_impl / refit_lbvh in float32"""
    lo, hi = np.asarray(scene_lo, F), np.asarray(scene_hi, F)
    cc = (F(0.5) * lo + F(0.5) * hi).astype(F)
    hk = np.maximum((hi - cc).astype(F), (cc - lo).astype(F))
    half_ext = F(max(F(0.0), hk.max()))
    base = half_ext if (half_ext > 0 and np.isfinite(half_ext)) else F(1.0)
    out = np.zeros(8, F)
    out[0:3] = cc
    out[3] = F(base) / F(1023.0)
    for k in range(3):
        own = hk[k] > F(half_ext * F(2.0 ** -20)) and np.isfinite(hk[k])
        out[4 + k] = F(hk[k] if own else base) / F(1023.0)
    return out


def record_boxes(tw, pad_abs):
    """(lo[n, 3], hi[n, 3]) float32: lbvh_build.hip record_aabb of the records (words [n, 12])"""
    f = np.ascontiguousarray(tw, np.uint32).reshape(-1, 12).view(F)
    pa, e1, e2 = f[:, 0:3], f[:, 3:6], f[:, 6:9]
    pb, pc = (pa + e1).astype(F), (pa + e2).astype(F)
    lo = np.minimum(pa, np.minimum(pb, pc))
    hi = np.maximum(pa, np.maximum(pb, pc))
    pad = np.maximum((F(1e-5) * np.maximum(F(1.0), np.maximum(np.abs(lo), np.abs(hi)))).astype(F), F(pad_abs))
    return (lo - pad).astype(F), (hi + pad).astype(F)


def records_of(verts, idx, mat_ids, prims):
    """The TriRecord words [n, 12] of the triangles `prims` (slot order), k_prepare's"""
    v = np.asarray(verts, F).reshape(len(verts), -1)[:, :3]
    i = np.asarray(idx, np.int64).reshape(-1, 3)[np.asarray(prims, np.int64)]
    a, b, c = v[i[:, 0]], v[i[:, 1]], v[i[:, 2]]
    out = np.zeros((len(i), 12), np.uint32)
    f = out.view(F)
    f[:, 0:3], f[:, 3:6], f[:, 6:9] = a, (b - a).astype(F), (c - a).astype(F)
    out[:, 9] = np.asarray(prims, np.uint32)
    out[:, 10] = np.asarray(mat_ids, np.uint32)[np.asarray(prims, np.int64)]
    return out


# ---- layouts -----------------------------------------------------------------------------------------------------------------------

def children_of(what, words):
    """(children int32 [n, 2] with inner references as indices, raw child words uint32 [n, 2])"""
    if what == 1:
        raw = words.reshape(-1, 16)[:, 12:14]
    else:
        raw = words.reshape(-1, 8)[:, [3, 7]]
    raw = np.ascontiguousarray(raw, np.uint32)
    c = raw.view(np.int32).copy()
    if what == 3:
        c = np.where(c >= 0, c >> 5, c)
    return c, raw


def fp32_boxes(words):
    """(lo, hi) [n, 2, 3] float32 views of the fp32 nodes' child boxes"""
    f = np.ascontiguousarray(words, np.uint32).reshape(-1, 16).view(F)
    return np.stack([f[:, 0:3], f[:, 6:9]], axis=1), np.stack([f[:, 3:6], f[:, 9:12]], axis=1)


def half_planes(words):
    """(low halves, high halves) [n, 2, 3] float64 of an fp16 node array"""
    w = np.ascontiguousarray(words, np.uint32).reshape(-1, 8)
    lo, hi = halves(np.stack([w[:, 0:3], w[:, 4:7]], axis=1))
    return lo, hi


# ---- the radix tree of the Karras build -------------------------------------------------------------------------------------------

def radix_tree(codes):
    """Karras' radix tree over the keys code << 32 | slot (sorted, distinct): (first[m], last[m], children int32 [m, 2]) of its n - 1
    inner nodes, node 0 the root, numbered in the order they are opened; a child < 0 is the leaf ~slot."""
    n = len(codes)
    keys = (np.asarray(codes, np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    first, last, children = [0], [n - 1], [[0, 0]]
    todo = [0]
    while todo:
        i = todo.pop()
        a, b = first[i], last[i]
        diff = int(keys[a]) ^ int(keys[b])
        bit = diff.bit_length() - 1                          # the highest bit in which the range's keys differ: 63 - common prefix
        target = ((int(keys[a]) >> bit) | 1) << bit          # the first key of the range with that bit set
        split = a + int(np.searchsorted(keys[a:b + 1], np.uint64(target)))      # ranges [a, split - 1] and [split, b]
        for k, (x, y) in enumerate(((a, split - 1), (split, b))):
            if x == y:
                children[i][k] = ~x
            else:
                first.append(x); last.append(y); children.append([0, 0])
                children[i][k] = len(first) - 1
                todo.append(len(first) - 1)
    return np.array(first), np.array(last), np.array(children, np.int32).reshape(-1, 2)


# ---- the checks --------------------------------------------------------------------------------------------------------------------

def _check_records(rep, tw, sw, verts, idx, mat_ids, morton):
    n = tw.shape[0]
    prim = tw[:, 9].astype(np.int64)
    ok = True
    bad = np.flatnonzero(prim >= n)
    for s in bad:
        rep.add("prim out of range", "tris", s, values=int(prim[s]))
    cnt = np.bincount(prim[prim < n], minlength=n)
    if bad.size or (cnt != 1).any():
        ok = False
        for p in np.flatnonzero(cnt != 1):
            rep.add("prim not a permutation", "tris", int(np.flatnonzero(prim == p)[0]) if cnt[p] else -1, values="prim %d appears %d times" % (p, cnt[p]))
    if morton is not None:
        m = np.asarray(morton[1], np.int64)
        rep.add_where("slot order differs from pt_read_morton", "tris", prim != m, np.arange(n), lambda s: (int(prim[s]), int(m[s])))
    if not ok:
        return False
    want = records_of(verts, idx, mat_ids, prim)
    rep.add_where("record words differ from the caller's vertices", "tris", tw[:, 0:9] != want[:, 0:9], np.arange(n),
                  lambda s, w: "word %d: %#x, expected %#x" % (w, tw[s, w], want[s, w]))
    rep.add_where("material id", "tris", (tw[:, 10] & 0xFFFFFF) != want[:, 10], np.arange(n), lambda s: (int(tw[s, 10]), int(want[s, 10])))
    if sw is not None:
        rep.add_where("material id", "shade", (sw[:, 3] & 0xFFFFFF) != want[:, 10], np.arange(n), lambda s: (int(sw[s, 3]), int(want[s, 10])))
        f = tw.view(F).astype(np.float64)
        e1, e2 = f[:, 3:6], f[:, 6:9]
        j, k = [1, 2, 0], [2, 0, 1]
        t1, t2 = e1[:, j] * e2[:, k], e1[:, k] * e2[:, j]
        cr = t1 - t2
        ln = np.sqrt((cr * cr).sum(axis=1))
        live = ln > 0
        with np.errstate(all="ignore"):
            want_n = cr / ln[:, None]
            err = 2.0 ** -24 * (np.abs(t1) + np.abs(t2) + np.abs(cr))           # of each cross component: two products and a difference, half an ulp each
            bound = 4.0 * np.spacing(np.abs(want_n).astype(F)).astype(np.float64) + (err + np.abs(want_n) * (np.abs(want_n) * err).sum(axis=1)[:, None]) / ln[:, None]
            got = sw.view(F)[:, 0:3].astype(np.float64)
            miss = live[:, None] & ~(np.abs(got - want_n) <= bound)
        rep.add_where("shade normal", "shade", miss, np.arange(n), lambda s, a: (float(got[s, a]), float(want_n[s, a]), float(bound[s, a])))
    return True


def _topology(rep, name, children, empty, n_tris):
    """levels (list of node arrays per depth) or None where the references do not make a tree"""
    n = children.shape[0]
    ok = True
    for node, k in np.argwhere(empty):
        if not (n_tris == 1 and node == 0 and k == 1):
            rep.add("empty child box", name, node, k)
            ok = False
    if n_tris == 1 and not (n == 1 and empty[0, 1] and not empty[0, 0] and children[0, 0] == -1):
        rep.add("one-triangle node", name, 0, values=children[0].tolist())
        return None
    c = np.where(empty, np.int32(n + n_tris + 1), children)        # an empty child references nothing
    inner, leaf = (c >= 0) & ~empty, (c < 0) & ~empty
    far = (inner & (c >= n)) | (leaf & (~c >= n_tris))
    rep.add_where("child reference out of range", name, far, np.arange(n), lambda i, k: int(children[i, k]))
    if far.any():
        return None
    cnt_in = np.bincount(c[inner], minlength=n)
    cnt_leaf = np.bincount(~c[leaf], minlength=n_tris)
    if cnt_in[0] != 0:
        rep.add("node 0 is referenced", name, 0, values=int(cnt_in[0])); ok = False
    for i in np.flatnonzero(cnt_in[1:] != 1) + 1:
        rep.add("inner node referenced %s" % ("never" if cnt_in[i] == 0 else "more than once"), name, i, values=int(cnt_in[i])); ok = False
    for s in np.flatnonzero(cnt_leaf != 1):
        par = np.argwhere(leaf & (c == ~np.int32(s)))
        rep.add("leaf referenced %s" % ("never" if cnt_leaf[s] == 0 else "more than once"), name, par[0, 0] if len(par) else -1,
                par[0, 1] if len(par) else -1, values="slot %d, %d references" % (s, cnt_leaf[s])); ok = False
    if not ok:
        return None
    levels, frontier, seen = [], np.array([0], np.int64), 0
    while frontier.size and len(levels) <= n:
        levels.append(frontier)
        seen += frontier.size
        ch = c[frontier]
        frontier = ch[inner[frontier]].astype(np.int64)
    if seen != n:
        reached = np.zeros(n, bool)
        reached[np.concatenate(levels)] = True
        for i in np.flatnonzero(~reached):
            rep.add("not reachable from node 0", name, i)
        return None
    return levels


def _aggregate(children, empty, levels, leaf_lo, leaf_hi):
    """Bottom-up over the levels: expected child boxes (lo, hi [n, 2, 3] float32) and per child the leaves below it: count, lowest and
    highest slot, slot sum, slot square sum (uint64, wrapping), inner nodes"""
    n = children.shape[0]
    z = lambda dt: np.zeros((n, 2), dt)
    exp_lo, exp_hi = np.full((n, 2, 3), np.inf, F), np.full((n, 2, 3), -np.inf, F)
    cnt, smin, smax, ssum, ssq, inn = z(np.int64), z(np.int64), z(np.int64), z(np.uint64), z(np.uint64), z(np.int64)
    for lev in reversed(levels):
        for k in (0, 1):
            c = children[lev, k].astype(np.int64)
            live = ~empty[lev, k]
            isleaf = (c < 0) & live
            isin = (c >= 0) & live
            s = np.where(isleaf, ~c, 0)
            j = np.where(isin, c, 0)
            lo = np.where(isleaf[:, None], leaf_lo[s], np.minimum(exp_lo[j, 0], exp_lo[j, 1]))
            hi = np.where(isleaf[:, None], leaf_hi[s], np.maximum(exp_hi[j, 0], exp_hi[j, 1]))
            exp_lo[lev, k] = np.where(live[:, None], lo, F(np.inf))
            exp_hi[lev, k] = np.where(live[:, None], hi, F(-np.inf))
            su = s.astype(np.uint64)
            cnt[lev, k] = np.where(isleaf, 1, cnt[j].sum(axis=1)) * live
            smin[lev, k] = np.where(isleaf, s, smin[j].min(axis=1))
            smax[lev, k] = np.where(isleaf, s, smax[j].max(axis=1))
            ssum[lev, k] = np.where(isleaf, su, ssum[j, 0] + ssum[j, 1])
            ssq[lev, k] = np.where(isleaf, su * su, ssq[j, 0] + ssq[j, 1])
            inn[lev, k] = np.where(isin, 1 + inn[j].sum(axis=1), 0)
    return exp_lo, exp_hi, dict(cnt=cnt, smin=smin, smax=smax, ssum=ssum, ssq=ssq, inner=inn)


def _ulps(a, b):
    """signed distance b - a in float32 steps"""
    def order(x):
        u = np.asarray(x, F).reshape(-1).view(np.int32).astype(np.int64)
        return np.where(u < 0, -(u & 0x7FFFFFFF), u)
    return order(b) - order(a)


def _check_fp32(rep, words, exp_lo, exp_hi):
    lo, hi = fp32_boxes(words)
    nodes = np.arange(lo.shape[0])
    for got, want, side, sign in ((lo, exp_lo, "lo", 1), (hi, exp_hi, "hi", -1)):
        bad = got.view(np.uint32) != want.view(np.uint32)
        rep.add_where("fp32 %s plane" % side, "fp32", bad, nodes,
                      lambda i, k, a: "%r, expected %r: %d ulp %s" % (float(got[i, k, a]), float(want[i, k, a]), abs(int(_ulps(want[i, k, a], got[i, k, a])[0])),
                                                                      "inward" if sign * int(_ulps(want[i, k, a], got[i, k, a])[0]) > 0 else "outward"))


def _to_space(w, c, inv):
    with np.errstate(invalid="ignore"):
        return (w.astype(np.float64) - np.asarray(c, np.float64)) / np.asarray(inv, np.float64)


def _check_h16(rep, words, exp_lo, exp_hi, empty, hs):
    g_lo, g_hi = half_planes(words)
    nodes = np.arange(g_lo.shape[0])
    live = ~empty[:, :, None] & np.ones(3, bool)
    a_lo, a_hi = _to_space(exp_lo, hs[0:3], hs[3]), _to_space(exp_hi, hs[0:3], hs[3])
    with np.errstate(invalid="ignore"):
        rep.add_where("empty child is not +inf / -inf", "h16", ~live & ~((g_lo == np.inf) & (g_hi == -np.inf)), nodes, lambda i, k, a: (g_lo[i, k, a], g_hi[i, k, a]))
        rep.add_where("containment (lo)", "h16", live & ~(g_lo <= a_lo - np.abs(a_lo) * 2.0 ** -19), nodes, lambda i, k, a: "g %r, exact %r" % (g_lo[i, k, a], a_lo[i, k, a]))
        rep.add_where("containment (hi)", "h16", live & ~(g_hi >= a_hi + np.abs(a_hi) * 2.0 ** -19), nodes, lambda i, k, a: "g %r, exact %r" % (g_hi[i, k, a], a_hi[i, k, a]))
        for g, a, side in ((g_lo, a_lo, "lo"), (g_hi, a_hi, "hi")):
            bound = ulp16(np.where(live, g, 0.0)) + np.abs(a) * 2.0 ** -17
            rep.add_where("tightness (%s)" % side, "h16", live & ~(np.abs(g - a) <= bound), nodes,
                          lambda i, k, ax: "g %r, exact %r, bound %r" % (g[i, k, ax], a[i, k, ax], bound[i, k, ax]))
            rep.note_slack("h16", (np.abs(g - a) / bound)[live])


def _check_hc16(rep, words, raw, children, exp_lo, exp_hi, empty, hs):
    c, h = half_planes(words)
    nodes = np.arange(c.shape[0])
    live = ~empty[:, :, None] & np.ones(3, bool)
    a_lo, a_hi = _to_space(exp_lo, hs[0:3], hs[4:7]), _to_space(exp_hi, hs[0:3], hs[4:7])
    with np.errstate(invalid="ignore"):
        m = np.maximum(np.abs(a_lo), np.abs(a_hi))
        rep.add_where("empty child has h >= 0", "hc16", ~live & ~(h < 0), nodes, lambda i, k, a: h[i, k, a])
        rep.add_where("containment (lo)", "hc16", live & ~(c - h <= a_lo - m * 2.0 ** -19), nodes, lambda i, k, a: "c %r h %r, exact lo %r" % (c[i, k, a], h[i, k, a], a_lo[i, k, a]))
        rep.add_where("containment (hi)", "hc16", live & ~(c + h >= a_hi + m * 2.0 ** -19), nodes, lambda i, k, a: "c %r h %r, exact hi %r" % (c[i, k, a], h[i, k, a], a_hi[i, k, a]))
        cs, hsafe = np.where(live, c, 0.0), np.where(live, h, 0.0)
        half = (a_hi - a_lo) / 2
        rest = ulp16(cs) / 2 + m * 2.0 ** -17 + ulp16(hsafe)
        rep.add_where("tightness (h)", "hc16", live & ~(h <= half + rest), nodes, lambda i, k, a: "h %r, exact %r, allowance %r" % (h[i, k, a], half[i, k, a], rest[i, k, a]))
        rep.note_slack("hc16", ((h - half) / rest)[live])
        mid = (a_lo + a_hi) / 2
        rep.add_where("centre is not the nearest fp16", "hc16", live & ~(np.abs(c - mid) <= ulp16(cs) / 2 + m * 2.0 ** -21), nodes,
                      lambda i, k, a: "c %r, midpoint %r" % (c[i, k, a], mid[i, k, a]))
    want = np.where(children >= 0, children.astype(np.int64) << 5, children.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    rep.add_where("child word (inner references are index << 5)", "hc16", raw != want, nodes, lambda i, k: "%#x, expected %#x" % (raw[i, k], want[i, k]))


def _check_wide(rep, wr, tw, info, leaf_lo, leaf_hi, agg):
    n_rec, n = wr.shape[0], tw.shape[0]
    if n_rec != info.n_wrecs or n_rec != info.n_wnodes + n:
        rep.add("record count", "wide", -1, values=(n_rec, info.n_wrecs, info.n_wnodes, n))
        return
    f = wr.view(F)
    seen = np.zeros(n_rec, np.int64)
    is_node = np.zeros(n_rec, bool)
    levels, level = [], np.array([0], np.int64)
    k4 = np.arange(4)
    while level.size and len(levels) <= n_rec:
        np.add.at(seen, level, 1)
        w3 = wr[level, 3]
        n_in, n_ch, base = ((w3 >> 24) & 7).astype(np.int64), (w3 >> 27).astype(np.int64), wr[level, 4].astype(np.int64)
        bad = (n_ch < 1) | (n_ch > 4) | (n_in > n_ch) | (base + n_ch > n_rec) | (base < 1)
        rep.add_where("children block", "wide", bad, level, lambda i: "n_inner %d n_children %d base %d" % (n_in[i], n_ch[i], base[i]))
        level, n_in, n_ch, base = level[~bad], n_in[~bad], n_ch[~bad], base[~bad]
        is_node[level] = True
        levels.append(level)
        idx = base[:, None] + k4
        inner = k4 < n_in[:, None]
        np.add.at(seen, idx[(k4 < n_ch[:, None]) & ~inner], 1)
        level = idx[inner]
    rep.add_where("record reached %s" % "other than once", "wide", seen != 1, np.arange(n_rec), lambda r: int(seen[r]))
    if (seen != 1).any():
        return
    if len(levels) != info.wide_depth or int(is_node.sum()) != info.n_wnodes:
        rep.add("wide_depth / n_wnodes", "wide", -1, values=(len(levels), info.wide_depth, int(is_node.sum()), info.n_wnodes))
    tri_rec = np.flatnonzero(~is_node)
    prim = wr[tri_rec, 9].astype(np.int64)
    slot_of = np.empty(n, np.int64)
    slot_of[tw[:, 9].astype(np.int64)] = np.arange(n)
    if (prim >= n).any() or (np.bincount(prim[prim < n], minlength=n) != 1).any():
        rep.add("triangle records are not every triangle once", "wide", -1)
        return
    slot = slot_of[prim]
    rep.add_where("triangle record differs from its TriRecord", "wide", wr[tri_rec] != tw[slot], tri_rec, lambda r, w: "word %d: %#x, TriRecord %#x" % (w, wr[tri_rec[r], w], tw[slot[r], w]))
    own_lo, own_hi = np.full((n_rec, 3), np.inf, F), np.full((n_rec, 3), -np.inf, F)
    cnt, ssum, ssq = np.zeros(n_rec, np.int64), np.zeros(n_rec, np.uint64), np.zeros(n_rec, np.uint64)
    own_lo[tri_rec], own_hi[tri_rec], cnt[tri_rec] = leaf_lo[slot], leaf_hi[slot], 1
    ssum[tri_rec] = slot.astype(np.uint64)
    ssq[tri_rec] = slot.astype(np.uint64) ** 2
    big = max(1.0, float(np.abs(info.scene_lo).max()), float(np.abs(info.scene_hi).max()),
              float((np.asarray(info.scene_hi, np.float64) - np.asarray(info.scene_lo, np.float64)).max()))
    margin = big * K_MARGIN_REL
    sig = lambda c, s, q: (c.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ (s * np.uint64(0xC2B2AE3D27D4EB4F)) ^ q
    known = np.concatenate([sig(agg["cnt"], agg["ssum"], agg["ssq"]).reshape(-1), sig(np.ones(n, np.int64), np.arange(n, dtype=np.uint64), np.arange(n, dtype=np.uint64) ** 2)])
    for lev in reversed(levels):
        w3 = wr[lev, 3]
        n_ch, base = (w3 >> 27).astype(np.int64), wr[lev, 4].astype(np.int64)
        valid = k4 < n_ch[:, None]
        idx = np.where(valid, base[:, None] + k4, 0)
        b_lo = np.where(valid[:, :, None], own_lo[idx], F(np.inf))
        b_hi = np.where(valid[:, :, None], own_hi[idx], F(-np.inf))
        own_lo[lev], own_hi[lev] = b_lo.min(axis=1), b_hi.max(axis=1)
        cnt[lev] = np.where(valid, cnt[idx], 0).sum(axis=1)
        ssum[lev] = np.where(valid, ssum[idx], np.uint64(0)).sum(axis=1, dtype=np.uint64)
        ssq[lev] = np.where(valid, ssq[idx], np.uint64(0)).sum(axis=1, dtype=np.uint64)
        rep.add_where("child is no subtree of the two-child tree", "wide", valid & ~np.isin(sig(cnt[idx], ssum[idx], ssq[idx]), known), lev, lambda i, k: int(cnt[idx[i, k]]))
        e = np.stack([(w3 >> (8 * a)) & 255 for a in range(3)], axis=1).astype(np.int64)            # [m, 3]
        cell = np.ldexp(1.0, e - 127)
        origin = f[lev, 0:3].astype(np.float64)
        q_lo = np.stack([(wr[lev, 6 + a][:, None] >> (8 * k4)) & 255 for a in range(3)], axis=2).astype(np.float64)        # [m, 4, 3]
        q_hi = np.stack([(wr[lev, 9 + a][:, None] >> (8 * k4)) & 255 for a in range(3)], axis=2).astype(np.float64)
        d_lo, d_hi = origin[:, None, :] + cell[:, None, :] * q_lo, origin[:, None, :] + cell[:, None, :] * q_hi
        v3 = valid[:, :, None] & np.ones(3, bool)
        rep.add_where("unused slot is not lo 255 / hi 0", "wide", ~v3 & ~((q_lo == 255) & (q_hi == 0)), lev, lambda i, k, a: (q_lo[i, k, a], q_hi[i, k, a]))
        with np.errstate(invalid="ignore"):
            x_lo, x_hi = b_lo.astype(np.float64), b_hi.astype(np.float64)
            rep.add_where("containment (lo)", "wide", v3 & ~(d_lo <= x_lo - margin), lev, lambda i, k, a: "decoded %r, fp32 %r, margin %r" % (d_lo[i, k, a], x_lo[i, k, a], margin))
            rep.add_where("containment (hi)", "wide", v3 & ~(d_hi >= x_hi + margin), lev, lambda i, k, a: "decoded %r, fp32 %r, margin %r" % (d_hi[i, k, a], x_hi[i, k, a], margin))
            allow = cell[:, None, :] + 2 * margin + 0 * x_lo
            rep.add_where("tightness (lo)", "wide", v3 & ~(x_lo - d_lo <= allow), lev, lambda i, k, a: "decoded %r, fp32 %r, cell %r" % (d_lo[i, k, a], x_lo[i, k, a], cell[i, a]))
            rep.add_where("tightness (hi)", "wide", v3 & ~(d_hi - x_hi <= allow), lev, lambda i, k, a: "decoded %r, fp32 %r, cell %r" % (d_hi[i, k, a], x_hi[i, k, a], cell[i, a]))
            rep.note_slack("wide", np.maximum(x_lo - d_lo, d_hi - x_hi)[v3] / allow[v3])
        ext = (own_hi[lev].astype(np.float64) + margin) - origin
        small = (e - 127 > -100) & ~(255.0 * np.ldexp(1.0, e - 128) < ext)
        rep.add_where("exponent is not the smallest", "wide", small | ~(255.0 * cell >= ext), lev, lambda i, a: "e %d, extent %r" % (e[i, a] - 127, ext[i, a]))
        rep.add_where("origin above the lowest plane", "wide", ~(origin <= own_lo[lev].astype(np.float64) - margin), lev, lambda i, a: (origin[i, a], float(own_lo[lev[i], a])))


def _check_karras(rep, name, agg, children, codes):
    n_tris = len(codes)
    codes = np.asarray(codes, np.int64)
    rep.add_where("Morton codes are not sorted", "tris", codes[1:] < codes[:-1], np.arange(1, n_tris), lambda s: (int(codes[s - 1]), int(codes[s])))
    if (codes[1:] < codes[:-1]).any():
        return
    cnt, smin, smax = agg["cnt"].sum(axis=1), agg["smin"].min(axis=1), agg["smax"].max(axis=1)
    nodes = np.arange(children.shape[0])
    gap = cnt != smax - smin + 1
    rep.add_where("leaves are no contiguous slot range", name, gap, nodes, lambda i: "%d leaves in [%d, %d]" % (cnt[i], smin[i], smax[i]))
    first, last, _ = radix_tree(codes)
    want = set(zip(first.tolist(), last.tolist()))
    for i in np.flatnonzero(~gap):
        if (int(smin[i]), int(smax[i])) not in want:
            rep.add("range is none of the radix tree's", name, i, values=(int(smin[i]), int(smax[i])))
    have = set(zip(smin[~gap].tolist(), smax[~gap].tolist()))
    for r in sorted(want - have)[:rep.cap]:
        rep.add("radix-tree range is missing", name, -1, values=r)
    assert n_tris == len(first) + 1


def validate(arrays, info, verts, idx, mat_ids, morton=None, stack_entries=None, depth_first=None, cap=12):
    """See the module docstring.  morton: (codes_sorted, prims_sorted) of pt_read_morton, or None; stack_entries: pt_bvh_info's, or None;
    depth_first: True / False to hold the node numbering to pre-order or not, None to skip."""
    rep = Violations(cap)
    arrays = {k: np.ascontiguousarray(v, np.uint32).reshape(-1) for k, v in arrays.items()}
    n, n_nodes = int(info.n_tris), int(info.n_nodes)
    if n_nodes != max(n - 1, 1):
        rep.add("n_nodes", "info", -1, values=(n_nodes, n))
        return rep.finish()
    sizes = {1: n_nodes * 16, 2: n_nodes * 8, 3: n_nodes * 8, 4: int(info.n_wrecs) * 12, 5: n * 12, 6: n * 4}
    for k, a in arrays.items():
        if a.size != sizes[k]:
            rep.add("array size", NAMES[k], -1, values=(a.size, sizes[k]))
            return rep.finish()
    tw = arrays[5].reshape(n, 12)
    sw = arrays[6].reshape(n, 4) if 6 in arrays else None
    if not _check_records(rep, tw, sw, verts, idx, mat_ids, morton):
        return rep.finish()
    want_pad = pad_abs_of(verts)
    if F(info.pad_abs).view(np.uint32) != want_pad.view(np.uint32):
        rep.add("pad_abs", "info", -1, values=(float(info.pad_abs), float(want_pad)))
    leaf_lo, leaf_hi = record_boxes(tw, want_pad)
    want_lo, want_hi = leaf_lo.min(axis=0), leaf_hi.max(axis=0)
    for got, want, what in ((info.scene_lo, want_lo, "scene_lo"), (info.scene_hi, want_hi, "scene_hi")):
        rep.add_where(what, "info", np.asarray(got, F).view(np.uint32) != want.view(np.uint32), [-1] * 3, lambda a: (float(got[a]), float(want[a])))
    hs_want = hspace_of(want_lo, want_hi)
    hs = np.asarray(info.hspace, F)
    rep.add_where("HSpace", "info", hs.view(np.uint32) != hs_want.view(np.uint32), [-1] * 8,
                  lambda a: "%s: %r, expected %r" % (("cx", "cy", "cz", "inv_scale", "isx", "isy", "isz", "pad_")[a], float(hs[a]), float(hs_want[a])))
    hs64 = hs_want.astype(np.float64)

    first, levels, agg = None, None, None
    for what in (1, 2, 3):
        if what not in arrays:
            continue
        name = NAMES[what]
        children, raw = children_of(what, arrays[what])
        if what == 1:
            lo, hi = fp32_boxes(arrays[1])
            with np.errstate(invalid="ignore"):
                empty = ~(lo <= hi).all(axis=2)
        elif what == 2:
            g_lo, g_hi = half_planes(arrays[2])
            with np.errstate(invalid="ignore"):
                empty = ~(g_lo <= g_hi).all(axis=2)
        else:
            empty = (half_planes(arrays[3])[1] < 0).any(axis=2)
        if first is None:
            levels = _topology(rep, name, children, empty, n)
            if levels is None:
                return rep.finish()
            first = (name, children)
            depth = len(levels)
            if depth != info.max_depth:
                rep.add("max_depth", "info", 0, values="longest path %d inner nodes, max_depth %d" % (depth, info.max_depth))
            if stack_entries is not None and depth > stack_entries - 1:
                rep.add("stack_entries", "info", 0, values=(depth, stack_entries))
            exp_lo, exp_hi, agg = _aggregate(children, empty, levels, leaf_lo, leaf_hi)
            root_lo, root_hi = exp_lo[0].min(axis=0), exp_hi[0].max(axis=0)
            if not (np.array_equal(root_lo, want_lo) and np.array_equal(root_hi, want_hi)):
                rep.add("root union is not the scene box", name, 0, values=(root_lo.tolist(), root_hi.tolist()))
            if info.mode == 0 and n > 1 and morton is not None:
                _check_karras(rep, name, agg, children, morton[0])
            if depth_first is not None and n > 1:
                i = np.arange(n_nodes)
                pre = np.stack([i + 1, i + 1 + agg["inner"][:, 0]], axis=1)
                off = (children >= 0) & (children != pre)
                if depth_first:
                    rep.add_where("numbering is not depth first", name, off, i, lambda j, k: "child %d, pre-order %d" % (children[j, k], pre[j, k]))
        else:
            rep.add_where("topology differs from %s" % first[0], name, children != first[1], np.arange(n_nodes),
                          lambda i, k: "%d, there %d" % (children[i, k], first[1][i, k]))
            if (children != first[1]).any():
                continue
        if what == 1:
            _check_fp32(rep, arrays[1], exp_lo, exp_hi)
        elif what == 2:
            _check_h16(rep, arrays[2], exp_lo, exp_hi, np.isinf(exp_lo[:, :, 0]), hs64)
        else:
            _check_hc16(rep, arrays[3], raw, children, exp_lo, exp_hi, np.isinf(exp_lo[:, :, 0]), hs64)
    if 4 in arrays:
        if agg is None:
            rep.add("no two-child array to hold the wide records to", "wide", -1)
        else:
            _check_wide(rep, arrays[4].reshape(-1, 12), tw, info, leaf_lo, leaf_hi, agg)
    return rep.finish()


# ---- encoders: numpy ports of the builders' last steps (tests/test_tree_ref_host.py builds its reference trees with them) -----------

def encode_fp32(children, exp_lo, exp_hi):
    n = children.shape[0]
    out = np.zeros((n, 16), np.uint32)
    f = out.view(F)
    f[:, 0:3], f[:, 3:6], f[:, 6:9], f[:, 9:12] = exp_lo[:, 0], exp_hi[:, 0], exp_lo[:, 1], exp_hi[:, 1]
    out[:, 12:14] = children.view(np.uint32)
    return out


def encode_h16(children, exp_lo, exp_hi, hs):
    n = children.shape[0]
    out = np.zeros((n, 8), np.uint32)
    for k in (0, 1):
        for a in range(3):
            out[:, 4 * k + a] = pack_planes(exp_lo[:, k, a], exp_hi[:, k, a], hs[a], hs[3])
        out[:, 4 * k + 3] = children[:, k].view(np.uint32)
    return out


def encode_hc16(children, exp_lo, exp_hi, hs):
    n = children.shape[0]
    out = np.zeros((n, 8), np.uint32)
    for k in (0, 1):
        for a in range(3):
            out[:, 4 * k + a] = pack_centre_half(exp_lo[:, k, a], exp_hi[:, k, a], hs[a], hs[4 + a])
        c = children[:, k].astype(np.int64)
        out[:, 4 * k + 3] = np.where(c >= 0, c << 5, c & 0xFFFFFFFF).astype(np.uint32)
    return out


def encode_wide(children, exp_lo, exp_hi, tw, scene_lo, scene_hi):
    """wide_bvh.hip build_wide4 + encode(): (records [n_wrecs, 12], n_wnodes, wide_depth)"""
    import math
    big = max(1.0, float(np.abs(scene_lo).max()), float(np.abs(scene_hi).max()), float((np.asarray(scene_hi, np.float64) - np.asarray(scene_lo, np.float64)).max()))
    margin = big * K_MARGIN_REL

    def kids(i):
        out = []
        for k in (0, 1):
            lo, hi = exp_lo[i, k], exp_hi[i, k]
            if (lo <= hi).all():
                out.append((int(children[i, k]), lo.astype(np.float64), hi.astype(np.float64)))
        return out

    area = lambda it: (lambda d: d[0] * d[1] + d[1] * d[2] + d[2] * d[0])(it[2] - it[1])
    recs = [np.zeros(12, np.uint32)]
    todo = [(0, 0, 1)]
    n_wnodes = depth_max = 0
    while todo:
        node, rec, depth = todo.pop()
        items = kids(node)
        while len(items) < 4:
            inner = [(area(it), -k) for k, it in enumerate(items) if it[0] >= 0]
            if not inner:
                break
            pick = -max(inner)[1]
            c = kids(items[pick][0])
            items[pick] = c[0]
            if len(c) == 2:
                items.append(c[1])
        order = [it for it in items if it[0] >= 0]
        n_inner = len(order)
        order += [it for it in items if it[0] < 0]
        base = len(recs)
        recs += [None] * len(order)
        for k in range(len(order) - 1, -1, -1):
            if k < n_inner:
                todo.append((order[k][0], base + k, depth + 1))
            else:
                recs[base + k] = tw[~order[k][0]].copy()
        w = np.zeros(12, np.uint32)
        ebits = []
        for a in range(3):
            lo_min = min(it[1][a] - margin for it in order)
            hi_max = max(it[2][a] + margin for it in order)
            o = F(lo_min)
            if float(o) > lo_min:
                o = np.nextafter(o, F(-np.inf))
            w[a] = o.view(np.uint32)
            o = float(o)
            e = max(int(math.ceil(math.log2((hi_max - o) / 255.0))), -100)
            while True:
                scale = math.ldexp(1.0, e)
                ql, qh = [255] * 4, [0] * 4
                ok = True
                for k, it in enumerate(order):
                    l, h = it[1][a] - margin, it[2][a] + margin
                    a_l, a_h = max(math.floor((l - o) / scale), 0), math.ceil((h - o) / scale)
                    while a_l > 0 and o + a_l * scale > l:
                        a_l -= 1
                    while o + a_h * scale < h:
                        a_h += 1
                    if a_h > 255 or a_l > 255:
                        ok = False
                        break
                    ql[k], qh[k] = a_l, a_h
                if ok:
                    break
                e += 1
            ebits.append(e + 127)
            w[6 + a] = ql[0] | (ql[1] << 8) | (ql[2] << 16) | (ql[3] << 24)
            w[9 + a] = qh[0] | (qh[1] << 8) | (qh[2] << 16) | (qh[3] << 24)
        w[3] = ebits[0] | (ebits[1] << 8) | (ebits[2] << 16) | (n_inner << 24) | (len(order) << 27)
        w[4] = base
        recs[rec] = w
        n_wnodes += 1
        depth_max = max(depth_max, depth)
    return np.stack(recs).astype(np.uint32), n_wnodes, depth_max
