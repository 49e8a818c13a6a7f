// oracle/build_ref.cpp — sequential statement of the parallel reinsertion of csrc/lbvh_build.hip (section 13: build mode 2 above
// kOptimizeMaxTris triangles).  TEST INFRASTRUCTURE, NOT PRODUCT: loaded with ctypes by tests/build_ref.py, which holds the device's
// tree to this one word for word.  One thread, plain loops; built with -ffp-contract=off -fno-fast-math, so every fp32 expression
// below rounds as the same expression does on the device.
//
// A round:  find    every node x (not the root, not a child of the root) looks for the node y next to which it would hang best:
//                   walking up from its parent p, the pivot A is p, then p's parent, ...; at each pivot the subtree of A's child on the
//                   far side is searched depth first without a stack.  gain(x, y) = what the nodes between x and A lose when x leaves
//                   (p altogether) - area(y u x) - what the nodes between A and y grow by.
//           lock    key(x) = gain bits << 32 | x.  Per node the largest key over the moves that EDIT it (x, p, p's parent, x's sibling,
//                   y, y's parent) and the largest over the moves that insert THROUGH it (y's parent up to, not including, A).
//           winners a move whose key is the edit maximum of its six nodes and not below their through maximum, and not below the edit
//                   maximum of the nodes it inserts through.
//           apply   the sibling takes p's place, p becomes the node (y, x) where y was.  Winners' edit sets are disjoint: any order.
//           refit   boxes and heights bottom-up.
// Nodes carry the device's unified numbers: inner nodes 0 .. m-1 (root 0), leaf slot s = m + s.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#define BREF_API extern "C" __attribute__((visibility("default")))

namespace {

enum : uint32_t {                       // test-only switches: one rule altered each (tests/test_build_ref_host.py, sensitivity of the scenes)
    kNoThroughLocks = 1u,               // the winner check ignores the through words
    kKeyNodeFirst = 2u,                 // lock key = node << 32 | gain bits
    kNoSiblingExclusion = 4u,           // the sibling is a legal target at the first pivot
};

struct Box { float lo[3], hi[3]; };
inline float area(const Box& b) { const float x = b.hi[0] - b.lo[0], y = b.hi[1] - b.lo[1], z = b.hi[2] - b.lo[2]; return x * y + y * z + z * x; }
inline Box unite(const Box& a, const Box& b)
{ Box r; for (int k = 0; k < 3; k++) { r.lo[k] = fminf(a.lo[k], b.lo[k]); r.hi[k] = fmaxf(a.hi[k], b.hi[k]); } return r; }
inline float union_area(const Box& a, const Box& b)
{
    const float x = fmaxf(a.hi[0], b.hi[0]) - fminf(a.lo[0], b.lo[0]), y = fmaxf(a.hi[1], b.hi[1]) - fminf(a.lo[1], b.lo[1]), z = fmaxf(a.hi[2], b.hi[2]) - fminf(a.lo[2], b.lo[2]);
    return x * y + y * z + z * x;
}

struct Move { int target = -1, pivot = -1; float gain = 0.0f; };

struct Tree {
    uint32_t m = 0, n = 0;
    std::vector<int> parent;            // [m + n]
    std::vector<int> child;             // [2 m]
    std::vector<Box> box;               // [m + n]
    std::vector<float> height;          // [m + n], 0 for a leaf
    uint32_t max_level = 0, max_guard = 0, max_through = 0;      // the largest values the device's three loop caps (64, 2^20, 4096) were asked for

    int unified(int ref) const { return ref >= 0 ? ref : (int)m + ~ref; }
    int sibling(int x) const { const int p = parent[(size_t)x]; return child[2 * (size_t)p] == x ? child[2 * (size_t)p + 1] : child[2 * (size_t)p]; }

    void load(const uint32_t* words, uint32_t m_, uint32_t n_)
    {
        m = m_; n = n_;
        parent.assign((size_t)m + n, -1); child.assign(2 * (size_t)m, 0); box.assign((size_t)m + n, Box()); height.assign((size_t)m + n, 0.0f);
        for (uint32_t i = 0; i < m; i++) {
            const uint32_t* w = words + 16 * (size_t)i;
            float f[12]; int32_t c[2];
            memcpy(f, w, 48); memcpy(c, w + 12, 8);
            for (int k = 0; k < 2; k++) {
                const int u = unified(c[k]);
                child[2 * (size_t)i + k] = u;
                parent[(size_t)u] = (int)i;
                Box b;
                for (int a = 0; a < 3; a++) { b.lo[a] = f[6 * k + a]; b.hi[a] = f[6 * k + 3 + a]; }
                box[(size_t)u] = b;
            }
        }
        parent[0] = -1;
    }
    // boxes and heights of the inner nodes from the leaves; false where the references below the root are not a tree of all m + n nodes
    bool refit()
    {
        std::vector<int> order;
        order.reserve(m);
        order.push_back(0);
        size_t leaves = 0;
        for (size_t at = 0; at < order.size(); at++) {
            if (order.size() > m) return false;
            for (int k = 0; k < 2; k++) {
                const int c = child[2 * (size_t)order[at] + k];
                if (c < 0 || c >= (int)(m + n) || parent[(size_t)c] != order[at]) return false;
                if (c < (int)m) order.push_back(c); else leaves++;
            }
        }
        if (order.size() != m || leaves != n) return false;
        for (size_t at = order.size(); at-- > 0;) {
            const int i = order[at], a = child[2 * (size_t)i], b = child[2 * (size_t)i + 1];
            box[(size_t)i] = unite(box[(size_t)a], box[(size_t)b]);
            height[(size_t)i] = fmaxf(height[(size_t)a], height[(size_t)b]) + 1.0f;
        }
        return true;
    }
    double area_sum() const { double s = 0.0; for (uint32_t i = 0; i < m; i++) s += (double)area(box[i]); return s; }

    Move find(int x, uint32_t alter)
    {
        Move out;
        if (x == 0) return out;
        const int p = parent[(size_t)x];
        if (p <= 0) return out;                             // children of the root stay
        const Box b = box[(size_t)x];
        const float ab = area(b);
        float best = 0.0f; int best_y = -1, best_pivot = -1;
        const int sib = sibling(x);
        Box without = box[(size_t)sib];                     // what the node below the pivot keeps once x is gone
        float gain = area(box[(size_t)p]);                  // p disappears
        int cur = p, other = sib, piv = p;
        uint32_t level = 0;
        for (;; level++) {
            // depth first below `other`; induced = growth of the nodes from `other` down to the parent of `node`
            int node = other;
            float induced = 0.0f;
            bool down = true;
            uint32_t guard = 0;
            for (;; guard++) {
                if (down) {
                    const Box& nb = box[(size_t)node];
                    const float direct = union_area(nb, b);
                    const float g = gain - induced - direct;
                    const bool excluded = piv == p && node == sib && !(alter & kNoSiblingExclusion);
                    if (g > best && !excluded) { best = g; best_y = node; best_pivot = piv; }
                    const float growth = direct - area(nb);
                    if (node < (int)m && gain - (induced + growth) - ab > best) { induced += growth; node = child[2 * (size_t)node]; }
                    else down = false;
                }
                if (!down) {
                    if (node == other) break;
                    const int par = parent[(size_t)node];
                    if (child[2 * (size_t)par] == node) { node = child[2 * (size_t)par + 1]; down = true; }
                    else {
                        induced -= union_area(box[(size_t)par], b) - area(box[(size_t)par]);
                        if (induced < 0.0f) induced = 0.0f;
                        node = par;
                    }
                }
            }
            max_guard = std::max(max_guard, guard + 1u);
            const int a = parent[(size_t)cur];
            if (a < 0) break;
            if (cur != p) gain += area(box[(size_t)cur]) - area(without);
            other = child[2 * (size_t)a] == cur ? child[2 * (size_t)a + 1] : child[2 * (size_t)a];
            without = unite(without, box[(size_t)other]);
            cur = a; piv = a;
            if (gain - ab <= best) break;
        }
        max_level = std::max(max_level, level + 1u);        // pivots visited: the device stops at 64
        if (best_y >= 0 && best > 0.0f) { out.target = best_y; out.pivot = best_pivot; out.gain = best; }
        return out;
    }
    void edit_set(int x, int y, int e[6]) const
    {
        const int p = parent[(size_t)x];
        e[0] = x; e[1] = p; e[2] = parent[(size_t)p]; e[3] = sibling(x); e[4] = y; e[5] = parent[(size_t)y];
    }
    void write(uint32_t* words) const
    {
        for (uint32_t i = 0; i < m; i++) {
            uint32_t* w = words + 16 * (size_t)i;
            float f[12]; int32_t c[4] = {0, 0, 0, 0};
            for (int k = 0; k < 2; k++) {
                const int u = child[2 * (size_t)i + k];
                for (int a = 0; a < 3; a++) { f[6 * k + a] = box[(size_t)u].lo[a]; f[6 * k + 3 + a] = box[(size_t)u].hi[a]; }
                c[k] = u < (int)m ? u : ~(u - (int)m);
            }
            memcpy(w, f, 48); memcpy(w + 12, c, 16);
        }
    }
};

inline uint64_t key_of(float gain, int x, uint32_t alter)
{
    uint32_t bits; memcpy(&bits, &gain, 4);
    return (alter & kKeyNodeFirst) ? ((uint64_t)(uint32_t)x << 32) | bits : ((uint64_t)bits << 32) | (uint32_t)x;       // gains are positive: their bits order as they do
}

}  // namespace

// Best move of every node of the tree `nodes` (fp32 node layout, m = n - 1 inner nodes): target, pivot (unified numbers, -1: none) and gain,
// [m + n] each.  caps[3] = the largest pivot count, search step count and (0 here) through-path length any node needed.  0, or -1: no tree.
BREF_API int bref_find(const uint32_t* nodes, uint32_t m, uint32_t n, uint32_t alter, int32_t* target, int32_t* pivot, float* gain, uint32_t* caps)
{
    Tree t;
    t.load(nodes, m, n);
    if (!t.refit()) return -1;
    for (uint32_t x = 0; x < m + n; x++) { const Move mv = t.find((int)x, alter); target[x] = mv.target; pivot[x] = mv.pivot; gain[x] = mv.gain; }
    caps[0] = t.max_level; caps[1] = t.max_guard; caps[2] = 0;
    return 0;
}

// `rounds` rounds of reinsertion on the tree `nodes`.  Out, per round r = 0 .. rounds-1: the tree after it (nodes_out + r * 16 m words),
// winners[r], height[r + 1] and area[r + 1] (the float64 sum over the inner nodes in index order); height[0], area[0]: the tree as given.
// checks[5] = largest pivot count, search step count, through-path length; pairs of winners of one round that share an edited node;
// the first round (1-based) after which the references were no tree (0: none).  Returns the rounds done (it stops at a broken tree).
BREF_API int bref_reinsert(const uint32_t* nodes, uint32_t m, uint32_t n, uint32_t rounds, uint32_t alter, uint32_t* nodes_out,
                           uint32_t* winners, double* area_out, uint32_t* height, uint32_t* checks)
{
    Tree t;
    t.load(nodes, m, n);
    memset(checks, 0, 5 * sizeof(uint32_t));
    if (!t.refit()) { checks[4] = 1u; return 0; }
    area_out[0] = t.area_sum(); height[0] = (uint32_t)t.height[0];
    const size_t N = (size_t)m + n;
    std::vector<Move> mv(N);
    std::vector<uint64_t> lock_edit(N), lock_through(N);
    std::vector<uint32_t> used(N);
    std::vector<int> won;
    uint32_t done = 0;
    for (uint32_t r = 0; r < rounds; r++) {
        for (size_t x = 0; x < N; x++) mv[x] = t.find((int)x, alter);
        std::fill(lock_edit.begin(), lock_edit.end(), 0u); std::fill(lock_through.begin(), lock_through.end(), 0u);
        for (size_t x = 0; x < N; x++) {
            if (mv[x].target < 0) continue;
            const uint64_t key = key_of(mv[x].gain, (int)x, alter);
            int e[6]; t.edit_set((int)x, mv[x].target, e);
            for (int k = 0; k < 6; k++) if (e[k] >= 0) lock_edit[(size_t)e[k]] = std::max(lock_edit[(size_t)e[k]], key);
            uint32_t len = 0;
            for (int a = t.parent[(size_t)mv[x].target]; a != mv[x].pivot && a >= 0; a = t.parent[(size_t)a], len++) lock_through[(size_t)a] = std::max(lock_through[(size_t)a], key);
            t.max_through = std::max(t.max_through, len);
        }
        won.clear();
        for (size_t x = 0; x < N; x++) {
            if (mv[x].target < 0) continue;
            const uint64_t key = key_of(mv[x].gain, (int)x, alter);
            int e[6]; t.edit_set((int)x, mv[x].target, e);
            bool all = true;
            for (int k = 0; k < 6; k++) if (e[k] >= 0) all = all && lock_edit[(size_t)e[k]] == key && ((alter & kNoThroughLocks) || lock_through[(size_t)e[k]] <= key);
            if (!(alter & kNoThroughLocks))
                for (int a = t.parent[(size_t)mv[x].target]; a != mv[x].pivot && a >= 0; a = t.parent[(size_t)a]) all = all && lock_edit[(size_t)a] <= key;
            if (all) won.push_back((int)x);
        }
        std::fill(used.begin(), used.end(), 0u);
        for (const int x : won) {
            int e[6]; t.edit_set(x, mv[(size_t)x].target, e);
            for (int k = 0; k < 6; k++) {
                if (e[k] < 0) continue;
                bool again = false;
                for (int j = 0; j < k; j++) again = again || e[j] == e[k];        // (y's parent may be p's parent: one node, one move)
                if (!again && used[(size_t)e[k]]++ != 0u) checks[3]++;
            }
        }
        for (const int x : won) {
            const int y = mv[(size_t)x].target, p = t.parent[(size_t)x], g = t.parent[(size_t)p], sib = t.sibling(x);
            t.child[2 * (size_t)g + (t.child[2 * (size_t)g] == p ? 0 : 1)] = sib;
            t.parent[(size_t)sib] = g;
            const int yp = t.parent[(size_t)y];             // after the step above: it may be g
            t.child[2 * (size_t)yp + (t.child[2 * (size_t)yp] == y ? 0 : 1)] = p;
            t.parent[(size_t)p] = yp;
            t.child[2 * (size_t)p] = y; t.child[2 * (size_t)p + 1] = x;
            t.parent[(size_t)y] = p; t.parent[(size_t)x] = p;
        }
        winners[r] = (uint32_t)won.size();
        if (!t.refit()) { checks[4] = r + 1u; break; }
        t.write(nodes_out + (size_t)r * 16 * m);
        area_out[r + 1] = t.area_sum(); height[r + 1] = (uint32_t)t.height[0];
        done = r + 1u;
    }
    checks[0] = t.max_level; checks[1] = t.max_guard; checks[2] = t.max_through;
    return (int)done;
}
