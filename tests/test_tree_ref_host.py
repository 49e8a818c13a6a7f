"""tests/tree_ref.py, the validator of a built BVH, shown to pass what is right and to fail what is wrong — without a GPU.

Reference trees are built here in numpy (a median split over 300 random triangles of a non-cubic scene, a one-triangle and a
two-triangle scene, and a Karras radix tree over Morton codes with ties), encoded into all four node formats by tree_ref's numpy ports of
the encoders (pack_planes, pack_centre_half, build_wide4 + encode): the validator reports nothing.  Then one fault at a time is injected
and has to be reported at the node it was put in.  The ports of the two fp16 encoders are also held to the validator's bounds on 10^6
intervals — flat, at the rim |g| = 1023, next to zero — since the bounds are derived from the encoders' source, not measured."""
import copy

import numpy as np
import pytest

import tree_ref as tr

F = np.float32


# ---- reference trees ---------------------------------------------------------------------------------------------------------------

def _soup(n, seed=1, extent=(500.0, 200.0, 40.0), offset=(-120.0, 30.0, 700.0)):
    rng = np.random.default_rng(seed)
    c = rng.random((n, 1, 3)) * np.array(extent) + np.array(offset)
    t = c + rng.normal(scale=6.0, size=(n, 3, 3))
    v = np.zeros((3 * n, 4), F)
    v[:, :3] = t.reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), (rng.integers(0, 5, n)).astype(np.uint32)


def _median_tree(v, idx):
    """children int32 [n - 1, 2] (node 0 the root, pre-order) and the triangles in leaf order (the slots)"""
    cen = v[:, :3][idx.astype(np.int64)].mean(axis=1)
    children, prims = [], []

    def build(ids):
        if len(ids) == 1:
            prims.append(int(ids[0]))
            return ~(len(prims) - 1)
        me = len(children)
        children.append([0, 0])
        axis = int(np.argmax(cen[ids].max(axis=0) - cen[ids].min(axis=0)))
        ids = ids[np.argsort(cen[ids, axis], kind="stable")]
        h = len(ids) // 2
        children[me][0] = build(ids[:h])
        children[me][1] = build(ids[h:])
        return me

    n = len(idx)
    if n == 1:
        return np.array([[-1, -1]], np.int32), np.array([0])
    build(np.arange(n))
    return np.array(children, np.int32), np.array(prims)


class Tree:
    """arrays {1..6}, info, the scene: what validate() takes"""

    def __init__(self, v, idx, ids, children, prims, mode=2, codes=None):
        self.v, self.idx, self.ids = v, idx, ids
        n = len(idx)
        tw = tr.records_of(v, idx, ids, prims)
        f = tw.view(F).astype(np.float64)
        cr = np.cross(f[:, 3:6], f[:, 6:9])
        sw = np.zeros((n, 4), np.uint32)
        with np.errstate(all="ignore"):
            sw.view(F)[:, 0:3] = (cr / np.sqrt((cr * cr).sum(axis=1))[:, None]).astype(F)
        sw[:, 3] = tw[:, 10] | (1 << 26)                                    # a tag above the low 24 bits, as tag_shade_records leaves them
        pad = tr.pad_abs_of(v)
        leaf_lo, leaf_hi = tr.record_boxes(tw, pad)
        empty = np.zeros(children.shape, bool)
        if n == 1:
            empty[0, 1] = True
        rep = tr.Violations()
        levels = tr._topology(rep, "fp32", children, empty, n)
        assert levels is not None and not rep, rep
        exp_lo, exp_hi, _ = tr._aggregate(children, empty, levels, leaf_lo, leaf_hi)
        lo, hi = leaf_lo.min(axis=0), leaf_hi.max(axis=0)
        self._independent(v, idx, prims, children, exp_lo, exp_hi, len(levels), lo, hi)
        hs = tr.hspace_of(lo, hi)
        wide, n_wnodes, wide_depth = tr.encode_wide(children, exp_lo, exp_hi, tw, lo, hi)
        self.arrays = {1: tr.encode_fp32(children, exp_lo, exp_hi), 2: tr.encode_h16(children, exp_lo, exp_hi, hs),
                       3: tr.encode_hc16(children, exp_lo, exp_hi, hs), 4: wide, 5: tw, 6: sw}
        self.info = tr.Info(n_tris=n, n_nodes=len(children), max_depth=len(levels), mode=mode, pad_abs=pad, hspace=hs, scene_lo=lo, scene_hi=hi,
                            n_wrecs=len(wide), n_wnodes=n_wnodes, wide_depth=wide_depth, held=63)
        self.morton = (np.zeros(n, np.uint32) if codes is None else codes, prims.astype(np.uint32))
        self.children, self.exp_lo, self.exp_hi, self.levels = children, exp_lo, exp_hi, levels
        self.stack_entries = len(levels) + 1

    @staticmethod
    def _independent(v, idx, prims, children, exp_lo, exp_hi, depth, lo, hi):
        """The boxes, the depth and the scene box once more without tree_ref: triangle boxes by tests/refit_ref.py, a recursion per node"""
        import refit_ref
        t_lo, t_hi = refit_ref.triangle_boxes(v, idx)
        s_lo, s_hi = refit_ref.scene_box(v, idx)
        assert np.array_equal(s_lo, lo) and np.array_equal(s_hi, hi)

        def box(ref):
            if ref < 0:
                return t_lo[prims[~ref]], t_hi[prims[~ref]], 0
            got = [box(int(children[ref, k])) for k in (0, 1) if not (len(idx) == 1 and k == 1)]
            for k, (l, h, _) in enumerate(got):
                assert np.array_equal(l, exp_lo[ref, k]) and np.array_equal(h, exp_hi[ref, k]), (ref, k)
            return np.minimum.reduce([g[0] for g in got]), np.maximum.reduce([g[1] for g in got]), 1 + max(g[2] for g in got)

        assert box(0)[2] == depth

    def check(self, only=None, **kw):
        a = self.arrays if only is None else {k: self.arrays[k] for k in only}
        return tr.validate(a, self.info, self.v, self.idx, self.ids, morton=self.morton, stack_entries=self.stack_entries, **kw)

    def mutated(self):
        t = copy.copy(self)
        t.arrays = {k: a.copy() for k, a in self.arrays.items()}
        t.info = copy.deepcopy(self.info)
        return t


@pytest.fixture(scope="module")
def soup():
    v, idx, ids = _soup(300)
    children, prims = _median_tree(v, idx)
    return Tree(v, idx, ids, children, prims)


def _karras(n=300, seed=5):
    """(scene, sorted codes with ties, children) of the radix tree; the slots are the triangles in their own order"""
    v, idx, ids = _soup(n, seed)
    rng = np.random.default_rng(seed)
    codes = np.sort(rng.integers(0, 1 << 30, n)).astype(np.uint32)
    codes[40:90] = codes[40]                                               # fifty equal codes: the tie rule
    codes[200:203] = codes[200]
    codes = np.sort(codes)
    first, last, children = tr.radix_tree(codes)
    return v, idx, ids, codes, children, first, last


@pytest.fixture(scope="module")
def karras():
    v, idx, ids, codes, children, _, _ = _karras()
    return Tree(v, idx, ids, children, np.arange(len(idx)), mode=0, codes=codes)


def _hit(vs, array, node, check=""):
    return any(x.array == array and x.node == node and check in x.check for x in vs)


# ---- what is right passes ----------------------------------------------------------------------------------------------------------

def test_the_reference_trees_pass(soup, karras):
    for t in (soup, karras):
        vs = t.check()
        assert vs == [], vs
        for k in ("h16", "hc16", "wide"):
            assert 0.0 < vs.slack[k] <= 1.0
        print("slack as a share of the bound:", vs.slack)
    assert soup.info.scene_hi[0] - soup.info.scene_lo[0] > 2 * (soup.info.scene_hi[1] - soup.info.scene_lo[1])       # not cubic
    assert len({float(x) for x in soup.info.hspace[4:7]}) == 3


@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_triangles_pass(n):
    v, idx, ids = _soup(n, seed=9)
    children, prims = _median_tree(v, idx)
    t = Tree(v, idx, ids, children, prims)
    assert t.info.n_nodes == 1 and t.info.max_depth == 1
    for only in (None, (1, 5, 6), (2, 5), (3, 5), (1, 4, 5)):
        assert t.check(only) == []
    if n == 2:      # an empty child is accepted in the one-triangle scene only
        m = t.mutated()
        m.arrays[1].view(F)[0, 6:9], m.arrays[1].view(F)[0, 9:12] = np.inf, -np.inf
        assert _hit(m.check((1, 5)), "fp32", 0, "empty child")


def test_each_array_alone_passes(soup):
    for only in ((1, 5, 6), (2, 5, 6), (3, 5, 6), (1, 4, 5), (3, 4, 5)):
        assert soup.check(only) == []


# ---- what is wrong is reported, at its node ------------------------------------------------------------------------------------------

def _step16(word, high, direction):
    """the packed word with its low / high half moved one fp16 step towards +inf (direction > 0) or -inf"""
    h = np.array([(word >> 16) if high else (word & 0xFFFF)], np.uint16).view(np.float16)
    h = np.nextafter(h, np.float16(np.inf if direction > 0 else -np.inf))
    bits = int(h.view(np.uint16)[0])
    return np.uint32((int(word) & 0xFFFF) | (bits << 16)) if high else np.uint32((int(word) & 0xFFFF0000) | bits)


def test_h16_plane_one_step_inward(soup):
    for word, high, direction, check in ((0, False, +1, "containment (lo)"), (5, True, -1, "containment (hi)")):
        m = soup.mutated()
        m.arrays[2][0, word] = _step16(m.arrays[2][0, word], high, direction)
        vs = m.check()
        assert _hit(vs, "h16", 0, check) and len(vs) == 1, vs
        assert vs[0].child == word // 4 and vs[0].axis == word % 4


def test_h16_plane_one_step_outward_is_too_loose(soup):
    m = soup.mutated()
    m.arrays[2][0, 1] = _step16(_step16(m.arrays[2][0, 1], False, -1), False, -1)         # one step is the rounding's own; two are not
    vs = m.check()
    assert _hit(vs, "h16", 0, "tightness (lo)") and len(vs) == 1, vs


def test_half_extent_one_step_short(soup):
    m = soup.mutated()
    m.arrays[3][0, 0] = _step16(m.arrays[3][0, 0], True, -1)
    vs = m.check()
    assert _hit(vs, "hc16", 0, "containment") and all(x.node == 0 and x.child == 0 and x.axis == 0 for x in vs), vs


def test_centre_one_step_off(soup):
    c = tr.half_planes(soup.arrays[3])[0][0]                                # node 0: [2, 3]
    k, a = np.unravel_index(np.argmax(np.abs(c)), c.shape)
    for direction in (+1, -1):
        m = soup.mutated()
        m.arrays[3][0, 4 * k + a] = _step16(m.arrays[3][0, 4 * k + a], False, direction)
        vs = m.check()
        assert _hit(vs, "hc16", 0, "centre is not the nearest") and all(x.node == 0 and x.child == k and x.axis == a for x in vs), vs


@pytest.mark.parametrize("direction", ["inward", "outward"])
def test_fp32_plane_one_ulp_off(soup, direction):
    m = soup.mutated()
    f = m.arrays[1].view(F)
    f[5, 8] = np.nextafter(f[5, 8], F(np.inf if direction == "inward" else -np.inf))             # child 1's lo.z
    vs = m.check((1, 5, 6))
    assert len(vs) == 1 and _hit(vs, "fp32", 5, "fp32 lo plane") and vs[0].child == 1 and vs[0].axis == 2, vs
    assert "1 ulp " + direction in vs[0].values


def test_stale_box_left_at_its_parents_size(soup):
    m = soup.mutated()
    f = m.arrays[1].view(F)
    node = int(soup.levels[3][0])
    f[node, 0:3] = np.minimum(f[node, 0:3], f[node, 6:9])                   # child 0 keeps the union of both: conservative, and too big
    f[node, 3:6] = np.maximum(f[node, 3:6], f[node, 9:12])
    vs = m.check((1, 5, 6))
    assert vs and all(x.array == "fp32" and x.node == node and x.child == 0 and "outward" in x.values for x in vs), vs


def test_child_references_swapped_between_nodes(soup):
    leafy = [i for i in range(len(soup.children)) if soup.children[i, 0] < 0]
    i, j = leafy[0], leafy[-1]
    m = soup.mutated()
    w = m.arrays[1]
    w[i, 12], w[j, 12] = w[j, 12], w[i, 12]                                 # still a tree: the boxes no longer belong to the children
    vs = m.check((1, 5, 6), cap=10000)                                       # (every ancestor of the two has another box now)
    assert _hit(vs, "fp32", i, "plane") and _hit(vs, "fp32", j, "plane") and {x.node for x in vs} >= {i, j}, vs
    vs = m.check(cap=10000)                                                        # and the other arrays carry another topology
    assert _hit(vs, "h16", i, "topology differs") and _hit(vs, "hc16", j, "topology differs")


def test_leaf_referenced_twice_and_another_never(soup):
    leafy = [i for i in range(len(soup.children)) if soup.children[i, 1] < 0]
    i, j = leafy[2], leafy[7]
    m = soup.mutated()
    m.arrays[2][i, 7] = m.arrays[2][j, 7]
    vs = m.check((2, 5, 6))
    assert _hit(vs, "h16", -1, "leaf referenced never") and any("more than once" in x.check and x.node in (i, j) for x in vs), vs
    m = soup.mutated()
    inner = [k for k in range(len(soup.children)) if soup.children[k, 0] > 0]
    m.arrays[1][inner[3], 12] = m.arrays[1][inner[9], 12]
    vs = m.check((1, 5, 6))
    assert _hit(vs, "fp32", int(soup.children[inner[9], 0]), "more than once") and _hit(vs, "fp32", int(soup.children[inner[3], 0]), "never"), vs


def test_inner_reference_not_shifted_by_five(soup):
    node = next(i for i in range(len(soup.children)) if soup.children[i, 1] > 40)
    m = soup.mutated()
    m.arrays[3][node, 7] >>= 5
    assert _hit(m.check(), "hc16", node), m.check()
    assert any(x.array == "hc16" for x in m.check((3, 5, 6)))


def test_max_depth_one_too_small(soup):
    m = soup.mutated()
    m.info.max_depth -= 1
    vs = m.check()
    assert len(vs) == 1 and vs[0].check == "max_depth", vs
    m = soup.mutated()
    vs = tr.validate(m.arrays, m.info, m.v, m.idx, m.ids, stack_entries=m.info.max_depth)
    assert len(vs) == 1 and vs[0].check == "stack_entries", vs


def test_wide_byte_one_cell_inward(soup):
    m = soup.mutated()
    m.arrays[4][0, 6] += 1                                                  # root, child 0, lo.x
    vs = m.check()
    assert len(vs) == 1 and _hit(vs, "wide", 0, "containment (lo)") and vs[0].child == 0 and vs[0].axis == 0, vs
    m = soup.mutated()
    m.arrays[4][0, 10] -= 1 << 8                                            # child 1, hi.y
    vs = m.check()
    assert len(vs) == 1 and _hit(vs, "wide", 0, "containment (hi)") and vs[0].child == 1 and vs[0].axis == 1, vs
    m = soup.mutated()
    m.arrays[4][0, 9] += 2                                                  # two cells outward: too loose
    assert _hit(m.check(), "wide", 0, "tightness (hi)")
    m = soup.mutated()
    m.arrays[4][0, 3] += 1                                                  # the x exponent one too large: every plane still contains
    assert _hit(m.check(), "wide", 0, "exponent")


def test_wide_triangle_record_with_one_word_changed(soup):
    w = soup.arrays[4]
    is_node = np.zeros(len(w), bool)
    todo = [0]
    while todo:
        r = todo.pop()
        is_node[r] = True
        todo += [int(w[r, 4]) + k for k in range((int(w[r, 3]) >> 24) & 7)]
    rec = int(np.flatnonzero(~is_node)[17])
    m = soup.mutated()
    m.arrays[4][rec, 2] ^= 1
    vs = m.check()
    assert len(vs) == 1 and _hit(vs, "wide", rec, "triangle record differs"), vs


def test_isy_replaced_by_inv_scale(soup):
    m = soup.mutated()
    m.info.hspace = m.info.hspace.copy()
    m.info.hspace[5] = m.info.hspace[3]
    vs = m.check()
    assert len(vs) == 1 and vs[0].check == "HSpace" and "isy" in vs[0].values, vs
    m = soup.mutated()                                                      # ... and nodes encoded with it: boxes a few times too tall in y
    hs = m.info.hspace.copy()
    hs[5] = hs[3]
    m.arrays[3] = tr.encode_hc16(soup.children, soup.exp_lo, soup.exp_hi, hs)
    vs = m.check((3, 5, 6))
    assert vs and all(x.array == "hc16" and x.axis == 1 for x in vs if x.node >= 0), vs


def test_karras_split_one_position_off():
    v, idx, ids, codes, children, first, last = _karras()
    # a node i = ([a, s - 1], j = [s, b]) whose second child j = (~s, k = [s + 1, b]): rotated to i = (j = ([a, s - 1], ~s), k), the
    # split of i moves from s to s + 1.  Still a tree with contiguous ranges and exact boxes, but not the radix tree.
    for i in range(len(children)):
        j = children[i, 1]
        if j > 0 and children[j, 0] < 0 and children[j, 1] > 0:
            break
    else:
        raise AssertionError("no such node")
    ch = children.copy()
    left, s, k = ch[i, 0], ch[j, 0], ch[j, 1]
    ch[i] = (j, k)
    ch[j] = (left, s)
    t = Tree(v, idx, ids, ch, np.arange(len(idx)), mode=0, codes=codes)
    vs = t.check()
    assert _hit(vs, "fp32", j, "none of the radix tree's") and _hit(vs, "fp32", -1, "radix-tree range is missing") and len(vs) == 2, vs
    t.info.mode = 1                                                         # a PLOC tree is not held to it
    assert t.check() == []


def test_karras_range_with_a_hole(karras):
    t = karras
    i, j = [k for k in range(len(t.children)) if t.children[k, 0] < 0][:2]
    ch = t.children.copy()
    ch[i, 0], ch[j, 0] = ch[j, 0], ch[i, 0]
    m = Tree(t.v, t.idx, t.ids, ch, np.arange(len(t.idx)), mode=0, codes=t.morton[0])
    assert any("contiguous" in x.check for x in m.check())


def test_prim_id_duplicated(soup):
    m = soup.mutated()
    m.arrays[5][5, 9] = m.arrays[5][6, 9]
    vs = m.check()
    assert _hit(vs, "tris", 5, "prim not a permutation") and all(x.array == "tris" for x in vs), vs


def test_records_and_materials(soup):
    m = soup.mutated()
    m.arrays[5][11, 4] ^= 1                                                 # e1.y off by one ulp
    assert _hit(m.check(), "tris", 11, "record words")
    m = soup.mutated()
    m.arrays[6][12, 3] ^= 1
    vs = m.check()
    assert len(vs) == 1 and _hit(vs, "shade", 12, "material id"), vs
    m = soup.mutated()
    m.arrays[6].view(F)[13, 0:3] *= F(-1.0)
    assert _hit(m.check(), "shade", 13, "shade normal")
    m = soup.mutated()
    m.morton = (m.morton[0], m.morton[1][::-1].copy())
    assert any("pt_read_morton" in x.check for x in m.check())
    m = soup.mutated()
    m.info.pad_abs = F(m.info.pad_abs * 2)
    assert [x.check for x in m.check()] == ["pad_abs"]


def test_depth_first_numbering(soup):
    assert soup.check(depth_first=True) == []                                # _median_tree numbers in pre-order
    v, idx, ids, codes, children, _, _ = _karras()
    t = Tree(v, idx, ids, children, np.arange(len(idx)), mode=0, codes=codes)
    assert any("depth first" in x.check for x in t.check(depth_first=True))


# ---- the encoder ports meet the bounds they were derived to meet ----------------------------------------------------------------------

def _intervals(n, seed):
    """n intervals [lo, hi] in the node space: ends uniform, log-uniform down to 1e-9, zero and on the rim; widths zero (flat),
    log-uniform and uniform"""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 5, n)
    mag = 10.0 ** rng.uniform(-9, np.log10(1023.0), n) * rng.choice([-1.0, 1.0], n)
    a = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [rng.uniform(-1023, 1023, n), mag, np.zeros(n), -1023.0 * np.ones(n)], 1023.0 - 0 * mag)
    wk = rng.integers(0, 4, n)
    w = np.select([wk == 0, wk == 1, wk == 2], [np.zeros(n), 10.0 ** rng.uniform(-9, 3.3, n), rng.uniform(0, 2046, n)], 1e-3)
    lo = np.where(kind == 4, np.clip(a - w, -1023, 1023), a)
    hi = np.where(kind == 4, a, np.clip(a + w, -1023, 1023))
    return lo, hi


@pytest.mark.parametrize("centre,inv_scale", [((278.0, 273.5, -279.75), 556.03 / 1023.0), ((1e7, -3.0, 0.0), 2.0 ** -3), ((0.0, 1e-6, 4096.5), 3.1e-7)])
def test_encoder_ports_meet_the_bounds(centre, inv_scale):
    n = 1_000_000 // 6 // 3 * 6                                            # a third of 10^6 intervals per space, as [nodes, 2, 3]
    lo, hi = _intervals(n, seed=int(abs(centre[0])) % 97)
    hs = np.array(list(centre) + [inv_scale, inv_scale, inv_scale * 0.37, inv_scale * 2.0 ** -20, 0.0], F)
    c = hs[0:3].astype(np.float64)
    shape = (n // 6, 2, 3)
    for what, scales in (("h16", hs[[3, 3, 3]]), ("hc16", hs[4:7])):
        s = scales.astype(np.float64)
        w_lo = (c + lo.reshape(shape) * s).astype(F)                        # whatever fp32 planes these are: they are the boxes
        w_hi = np.maximum((c + hi.reshape(shape) * s).astype(F), w_lo)
        children = np.zeros((shape[0], 2), np.int32)
        rep = tr.Violations()
        empty = np.zeros((shape[0], 2), bool)
        if what == "h16":
            tr._check_h16(rep, tr.encode_h16(children, w_lo, w_hi, hs), w_lo, w_hi, empty, hs.astype(np.float64))
        else:
            words = tr.encode_hc16(children, w_lo, w_hi, hs)
            tr._check_hc16(rep, words, words[:, [3, 7]], children, w_lo, w_hi, empty, hs.astype(np.float64))
        print(what, "largest slack as a share of the bound: %.4f" % rep.slack[what])
        assert rep == [], rep[:5]
        assert 0.5 < rep.slack[what] <= 1.0                                 # and the bound is no idle one


def _normals_fp32(tw):
    """pt_device.h normalize(cross(e1, e2)) operation for operation in float32 (the build is compiled without contraction)"""
    f = tw.view(F)
    e1, e2 = f[:, 3:6], f[:, 6:9]
    j, k = [1, 2, 0], [2, 0, 1]
    c = ((e1[:, j] * e2[:, k]).astype(F) - (e1[:, k] * e2[:, j]).astype(F)).astype(F)
    sq = (c * c).astype(F)
    d = ((sq[:, 0] + sq[:, 1]).astype(F) + sq[:, 2]).astype(F)
    with np.errstate(all="ignore"):
        return (c * (F(1.0) / np.sqrt(d).astype(F)).astype(F)[:, None]).astype(F)


@pytest.mark.parametrize("scale", [300.0, 4.0, 0.05])
def test_normal_bound_holds_for_an_fp32_evaluation(scale):
    """The shade-normal bound is met by a plain fp32 evaluation of the device's own expression on 10^5 triangles, down to slivers of a
    ten-thousandth of their distance from the origin, whose cross products cancel almost entirely"""
    n = 100000
    rng = np.random.default_rng(int(scale * 100))
    t = rng.uniform(20.0, 530.0, (n, 1, 3)) + rng.normal(scale=scale, size=(n, 3, 3))
    v = np.zeros((3 * n, 4), F)
    v[:, :3] = t.reshape(-1, 3)
    idx, ids = np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), np.zeros(n, np.uint32)
    tw = tr.records_of(v, idx, ids, np.arange(n))
    sw = np.zeros((n, 4), np.uint32)
    sw.view(F)[:, 0:3] = _normals_fp32(tw)
    rep = tr.Violations()
    assert tr._check_records(rep, tw, sw, v, idx, ids, None) and rep == [], rep[:4]
    if scale == 4.0:        # ordinary triangles: the cancellation term is a few ulp, and a component off by 1e-4 of itself is reported
        sw.view(F)[7, 1] *= F(1.0001)
        tr._check_records(rep, tw, sw, v, idx, ids, None)
        assert len(rep) == 1 and _hit(rep, "shade", 7, "shade normal") and rep[0].child == 1, rep
